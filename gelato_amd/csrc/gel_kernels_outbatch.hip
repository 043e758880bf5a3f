// gel_kernels_outbatch.hip -- the post-processing table of a BATCH of decision vectors with its Monte-Carlo envelope and the peaks
// of every flight (gel_output_table_batch*).  The row is output_row (gel_output_row.h), the function output_kernel
// calls for one vector: same expressions, same bits.
//
// Four kernels:
//   outbatch_rows_kernel   table and / or peaks.  One workgroup (one wavefront) = one vector, which walks its nodes in tiles of 64;
//                          a lane forms one row straight into the LDS tile [64][34] (no row is held in registers: 110-odd VGPRs
//                          as in output_kernel), the workgroup then stores the tile's selected columns -- 64 consecutive nodes of a
//                          vector are ONE contiguous piece of out -- as whole lines, and lane j scans selected column j of the tile
//                          in ascending node order for the vector's peaks (running minimum / maximum in registers; nothing of a
//                          table is read back).
//   outbatch_env_kernel    envelope partials of a call WITHOUT a table.  One workgroup (one wavefront) = (block of kEnvBlock consecutive vectors, 8 consecutive
//                          nodes); its 64 lanes form the rows of 8 vectors x 8 nodes per step into the LDS tile, then every
//                          (node, column) pair -- 8 ncols of them, up to five per lane, statistics in registers -- takes the step's 8
//                          vectors in ascending order: Welford's update.  32 steps, one partial [8] per pair.  No table is written.
//   outbatch_env_table_kernel  the same partials of a call WITH a table, read from it: one lane per (node, column), the block's
//                          vectors in ascending order through the same update -- the same bits, no second pass over the rows.
//   outbatch_merge_kernel  one lane per (node, column): the partials of the blocks in ascending order, Chan's merge, the envelope.
// No atomics; the order of every floating-point operation is a function of the vector index alone.  fp64 throughout.
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_output_row.h"
#include "gel_outbatch.h"

namespace gel {

namespace {
__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) <= 1.79769313486231570815e308; }

// row (vector b, node i) into dst[0 .. kOutputColumns): a row of the LDS tile; the columns of a part the call leaves out stay stale
// there and are never read
// kEns = 1 (gel_output_table_batch_ensemble*; with kDisp only, the other instantiations do not read Ens): the row's wind comes from
// the table vector b is assigned (ens_lane_tables: global memory), through the same wind_ned2 of output_row; A.disp may then be
// null: factors of one.  An int like prop_kernel's, not a branch inside the dispersed instantiation: with both rows in one kernel
// the dispersed call without an ensemble was 2 - 3 % slower than before.
template <bool kDisp, int kEns = 0>
__device__ __forceinline__ void row_to_tile(const ProblemDev& P, const Tables& tb, const OutBatchArgs& A, const EnsDev& Ens, long long b,
                                            int i, double* __restrict__ dst) {
  const int M = P.M, N = P.N;
  // the node's phase: section s owns the state nodes xa_s .. xa_s + n_s (output_result.py:121-143)
  int sec = 0;
  for (int s = 1; s < P.S; s++)
    if (i >= load_const(&P.phases[s].xa)) sec = s;
  PhaseDev ph = P.phases[sec];
  const double* const xb = A.x + (size_t)b * P.nvars;
  double t;
  if (A.tx) t = A.tx[(size_t)b * M + i];
  else {
    // node_times of gelato_amd/output_result.py, operation for operation: (tau_x (tf - to) / 2 + (tf + to) / 2) unit_t
    const int k = i - ph.xa;
    const double to = xb[11 * M + 2 * N + sec], tf = xb[11 * M + 2 * N + sec + 1];
    const double tau_x = (k == 0) ? -1.0 : P.tau[ph.toff + k - 1];
    const double p1 = tau_x * (tf - to);
    const double h1 = p1 / 2, h2 = (tf + to) / 2;
    const double sum = h1 + h2;
    t = sum * P.ut;
  }
  double fw = 1.0;
  if (kDisp && (!kEns || A.disp)) {   // (null only under an ensemble)
    const double* const fac = A.disp + ((size_t)b * P.S + sec) * 4;   // thrust, (mass flow: no reader here), reference area, wind
    ph.thrust = ph.thrust * fac[0];
    ph.area = ph.area * fac[2];
    fw = fac[3];
  }
  if constexpr (kEns) {
    const Tables tbe = ens_lane_tables(P, tb, Ens, Ens.member[b]);
    output_row<true>(P, tbe, ph, M, i, xb, t, A.lat0, A.lon0, dst, A.cols.parts, fw);
  } else output_row<kDisp>(P, tb, ph, M, i, xb, t, A.lat0, A.lon0, dst, A.cols.parts, fw);
}

// the column map col[j] = gel_output_column of selected column j into LDS (a lane cannot index the kernel argument by its id
// without a copy of it in scratch); the caller's next barrier publishes it
__device__ __forceinline__ void stage_colmap(const OutColsDev& C, int* cmap) {
  int mine = 0;
#pragma unroll
  for (int c = 0; c < kOutputColumns; c++)
    if ((int)threadIdx.x == c) mine = C.col[c];
  if ((int)threadIdx.x < kOutputColumns) cmap[threadIdx.x] = mine;
}
constexpr int kW = kOutputColumns;   // doubles per row of the tile

// the running statistics of one (node, column) pair inside a block of vectors, and the one place their arithmetic is written
struct EnvStat { double mean, m2, vmin, vmax; int cnt, amin, amax, fnf; };
__device__ __forceinline__ void env_init(EnvStat& e) { e.mean = e.m2 = e.vmin = e.vmax = 0.0; e.cnt = 0; e.amin = e.amax = e.fnf = -1; }
__device__ __forceinline__ void env_update(EnvStat& e, double v, int b) {
  if (!finite_d(v)) { if (e.fnf < 0) e.fnf = b; return; }
  // Welford: n += 1; d = v - mean; mean += d / n; m2 = fma(d, v - mean, m2)
  e.cnt += 1;
  const double d = v - e.mean;
  const double q = d / (double)e.cnt;
  e.mean = e.mean + q;
  const double d2 = v - e.mean;
  e.m2 = __builtin_fma(d, d2, e.m2);
  if (e.amin < 0 || v < e.vmin) { e.vmin = v; e.amin = b; }
  if (e.amax < 0 || v > e.vmax) { e.vmax = v; e.amax = b; }
}
__device__ __forceinline__ void env_store(const EnvStat& e, double* __restrict__ w) {
  w[0] = (double)e.cnt; w[1] = e.mean; w[2] = e.m2; w[3] = e.vmin; w[4] = e.vmax;
  w[5] = (double)e.amin; w[6] = (double)e.amax; w[7] = (double)e.fnf;
}
}  // namespace

template <bool kDisp, int kEns = 0>
__global__ __launch_bounds__(64) void outbatch_rows_kernel(ProblemDev P, OutBatchArgs A, double* __restrict__ out,
                                                           double* __restrict__ peaks, EnsDev Ens) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds);
  double* const tile = lds + ((table_doubles(P.Kw, P.Kc) + 1) & ~1);
  int* const cmap = reinterpret_cast<int*>(tile + 64 * kW);
  stage_colmap(A.cols, cmap);
  const long long b = blockIdx.x;
  const int lane = threadIdx.x, M = P.M, nc = A.cols.ncols;
  double pmin = 0.0, pmax = 0.0;
  int imin = -1, imax = -1;
  for (int t0 = 0; t0 < M; t0 += 64) {
    const int nrows = min(64, M - t0);
    if (lane < nrows) row_to_tile<kDisp, kEns>(P, tb, A, Ens, b, t0 + lane, tile + lane * kW);
    __syncthreads();
    if (out) {
      double* const dst = out + ((size_t)b * M + t0) * nc;
      for (int k = lane; k < nrows * nc; k += 64) {
        const int r = k / nc, j = k - r * nc;
        dst[k] = tile[r * kW + cmap[j]];
      }
    }
    if (peaks && lane < nc) {
      const int c = cmap[lane];
      for (int r = 0; r < nrows; r++) {
        const double v = tile[r * kW + c];
        if (!finite_d(v)) continue;
        if (imin < 0 || v < pmin) { pmin = v; imin = t0 + r; }
        if (imax < 0 || v > pmax) { pmax = v; imax = t0 + r; }
      }
    }
    __syncthreads();
  }
  if (peaks && lane < nc) {
    double* const pk = peaks + ((size_t)b * nc + lane) * kPeakNStat;
    pk[0] = (imin < 0) ? __builtin_nan("") : pmin;
    pk[1] = (double)imin;
    pk[2] = (imax < 0) ? __builtin_nan("") : pmax;
    pk[3] = (double)imax;
  }
}

constexpr int kEnvPairs = (kEnvNodes * kOutputColumns + 63) / 64;   // (node, column) pairs per lane: 5
template <bool kDisp, int kEns = 0>
__global__ __launch_bounds__(64) void outbatch_env_kernel(ProblemDev P, OutBatchArgs A, int ngroups, double* __restrict__ ws, EnsDev Ens) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds);
  double* const tile = lds + ((table_doubles(P.Kw, P.Kc) + 1) & ~1);
  int* const cmap = reinterpret_cast<int*>(tile + 64 * kW);
  stage_colmap(A.cols, cmap);
  const int blk = blockIdx.x / ngroups, grp = blockIdx.x - blk * ngroups;
  const int lane = threadIdx.x, M = P.M, nc = A.cols.ncols, B = A.B;
  const int vv = lane >> 3, i = grp * kEnvNodes + (lane & 7);
  const int npairs = kEnvNodes * nc;
  EnvStat es[kEnvPairs];
#pragma unroll
  for (int j = 0; j < kEnvPairs; j++) env_init(es[j]);
  const int b0 = blk * kEnvBlock;
  for (int st = 0; st < kEnvBlock / 8; st++) {
    const int bs = b0 + st * 8;      // first vector of the step
    if (bs >= B) break;
    const int nv = min(8, B - bs);
    if (vv < nv && i < M) row_to_tile<kDisp, kEns>(P, tb, A, Ens, bs + vv, i, tile + lane * kW);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kEnvPairs; j++) {
      const int p = lane + 64 * j;
      if (p >= npairs) continue;
      const int nn = p / nc, c = cmap[p - nn * nc];
      if (grp * kEnvNodes + nn >= M) continue;
      for (int r = 0; r < nv; r++) env_update(es[j], tile[(r * 8 + nn) * kW + c], bs + r);   // ascending vector index
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kEnvPairs; j++) {
    const int p = lane + 64 * j;
    if (p >= npairs) continue;
    const int nn = p / nc, c = p - nn * nc, i2 = grp * kEnvNodes + nn;
    if (i2 >= M) continue;
    env_store(es[j], ws + (((size_t)blk * M + i2) * nc + c) * kEnvNStat);
  }
}

// the same partials out of a table the call has just written (out != NULL): one lane = one (node, column) pair, which takes the
// block's vectors in ascending order -- the same env_update in the same order, hence the same bits -- and reads whole lines (the
// pairs of a vector are contiguous in out); no rows are formed a second time
__global__ __launch_bounds__(256) void outbatch_env_table_kernel(int B, long long npairs, int ptiles, const double* __restrict__ table,
                                                                 double* __restrict__ ws) {
  const int blk = blockIdx.x / ptiles;
  const long long p = (long long)(blockIdx.x - blk * ptiles) * 256 + threadIdx.x;
  if (p >= npairs) return;
  EnvStat e;
  env_init(e);
  const int b0 = blk * kEnvBlock, b1 = min(B, b0 + kEnvBlock);
  for (int b = b0; b < b1; b++) env_update(e, table[(size_t)b * npairs + p], b);
  env_store(e, ws + ((size_t)blk * npairs + p) * kEnvNStat);
}

__global__ __launch_bounds__(256) void outbatch_merge_kernel(long long npairs, int nblk, const double* __restrict__ ws,
                                                             double* __restrict__ env) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npairs) return;
  double n = 0.0, mean = 0.0, m2 = 0.0, vmin = 0.0, vmax = 0.0, amin = -1.0, amax = -1.0, fnf = -1.0;
  for (int k = 0; k < nblk; k++) {   // ascending block order
    const double* const w = ws + ((size_t)k * npairs + p) * kEnvNStat;
    if (fnf < 0.0 && w[7] >= 0.0) fnf = w[7];
    const double nb = w[0];
    if (nb == 0.0) continue;
    if (n == 0.0) { n = nb; mean = w[1]; m2 = w[2]; vmin = w[3]; vmax = w[4]; amin = w[5]; amax = w[6]; continue; }
    // Chan: nt = n + nb; d = mean_b - mean; mean += d (nb / nt); m2 = (m2 + m2_b) + (d d) (n nb / nt)
    const double nt = n + nb, d = w[1] - mean;
    const double fb = nb / nt, fab = n * nb / nt;
    const double dm = d * fb;
    mean = mean + dm;
    const double s2 = m2 + w[2], dd = d * d;
    const double t2 = dd * fab;
    m2 = s2 + t2;
    n = nt;
    if (w[3] < vmin) { vmin = w[3]; amin = w[5]; }
    if (w[4] > vmax) { vmax = w[4]; amax = w[6]; }
  }
  double* const e = env + (size_t)p * kEnvNStat;
  const double nan = __builtin_nan("");
  const bool none = (n == 0.0);
  e[0] = n; e[1] = none ? nan : mean; e[2] = none ? nan : m2; e[3] = none ? nan : vmin; e[4] = none ? nan : vmax;
  e[5] = amin; e[6] = amax; e[7] = fnf;
}

hipError_t launch_outbatch_rows(const ProblemDev& P, const OutBatchArgs& A, const EnsDev& ens, double* d_out, double* d_peaks,
                                hipStream_t s) {
  if (A.B <= 0 || (!d_out && !d_peaks)) return hipSuccess;
  const size_t lds = outbatch_lds_bytes(P.Kw, P.Kc);
  if (lds > kLaunchMaxLds) return hipErrorInvalidValue;
  auto* const kern = ens.tables ? outbatch_rows_kernel<true, 1> : A.disp ? outbatch_rows_kernel<true> : outbatch_rows_kernel<false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)A.B), dim3(64), lds, s, P, A, d_out, d_peaks, ens);
  return hipGetLastError();
}

hipError_t launch_outbatch_env(const ProblemDev& P, const OutBatchArgs& A, const EnsDev& ens, const double* d_table, double* d_ws,
                               double* d_env, hipStream_t s) {
  const int nblk = (A.B + kEnvBlock - 1) / kEnvBlock, ngroups = (P.M + kEnvNodes - 1) / kEnvNodes;
  const long long npairs = (long long)P.M * A.cols.ncols;
  if (nblk > 0 && d_table) {
    const long long ptiles = (npairs + 255) / 256, grid = nblk * ptiles;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(outbatch_env_table_kernel, dim3((unsigned)grid), dim3(256), 0, s, A.B, npairs, (int)ptiles, d_table, d_ws);
    if (const hipError_t e = hipGetLastError()) return e;
  } else if (nblk > 0) {
    const size_t lds = outbatch_lds_bytes(P.Kw, P.Kc);
    const long long grid = (long long)nblk * ngroups;
    if (lds > kLaunchMaxLds || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    auto* const kern = ens.tables ? outbatch_env_kernel<true, 1> : A.disp ? outbatch_env_kernel<true> : outbatch_env_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64), lds, s, P, A, ngroups, d_ws, ens);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(outbatch_merge_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, s, npairs, nblk, d_ws, d_env);
  return hipGetLastError();
}

}  // namespace gel
