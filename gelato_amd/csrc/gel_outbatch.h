// gel_outbatch.h -- the batched post-processing table (gel_output_table_batch*): what host and kernels share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gel_device.h"
#include "gel_launch.h"
#include "gel_ensemble.h"

namespace gel {

constexpr int kEnvNStat = 8;     // count, mean, m2, min, max, argmin, argmax, first_nonfinite (GEL_ENV_NSTAT)
constexpr int kPeakNStat = 4;    // min, node of min, max, node of max (GEL_PEAK_NSTAT)
constexpr int kEnvBlock = 256;   // vectors per envelope partial: block k = vectors 256 k .. 256 k + 255 (the stated reduction order)
constexpr int kEnvNodes = 8;     // nodes per workgroup of outbatch_env_kernel (8 nodes x 8 vectors = its 64 lanes)

// the selected columns: col[j] = the gel_output_column at place j of a row of the call's outputs (j < ncols)
struct OutColsDev {
  int32_t ncols;
  uint32_t parts;            // kRow* (gel_output_row.h): what the selected columns need
  int8_t col[kOutputColumns];
};

struct OutBatchArgs {
  int32_t B;
  const double* x;       // [B][nvars]
  const double* tx;      // [B][M] seconds, or null: from the vector's knots and the handle's tau
  const double* disp;    // [B][S][4] or null
  double lat0, lon0;
  OutColsDev cols;
};

// LDS of the two row kernels: the staged tables (padded to an even count), behind them the row tile [64][kOutputColumns] -- every
// row full width, whatever the call selects -- and the column map (kOutputColumns ints); the envelope keeps nothing else there
// (its running statistics are registers)
inline size_t outbatch_lds_bytes(int Kw, int Kc) {
  return sizeof(double) * (padded_table_doubles(Kw, Kc) + 64 * (size_t)kOutputColumns + (kOutputColumns + 1) / 2);
}
// doubles of the envelope partials of a call: [blocks][M][ncols][kEnvNStat]
inline size_t outbatch_ws_doubles(int B, int M, int ncols) {
  return (size_t)((B + kEnvBlock - 1) / kEnvBlock) * (size_t)M * (size_t)ncols * kEnvNStat;
}

// table [B][M][ncols] and / or peaks [B][ncols][4] (either may be null, not both): one workgroup per vector
// ens: the wind ensemble with the assignment of all B vectors, or ens.tables == null (the same for launch_outbatch_env); with an
// ensemble the kernels' kEns instantiation runs, with factors of one where A.disp is null
hipError_t launch_outbatch_rows(const ProblemDev& P, const OutBatchArgs& A, const EnsDev& ens, double* d_out, double* d_peaks,
                                hipStream_t s);
// envelope [M][ncols][8] through the partials ws (outbatch_ws_doubles).  d_table = the [B][M][ncols] table launch_outbatch_rows has
// written on the same stream for the same arguments: the partials are read from it; null: the rows are formed again, nothing of a
// table is written or read.  The same bits either way.
hipError_t launch_outbatch_env(const ProblemDev& P, const OutBatchArgs& A, const EnsDev& ens, const double* d_table, double* d_ws,
                               double* d_env, hipStream_t s);

}  // namespace gel
