// gel_kernels_aerorows.hip -- the aero path constraints' rows on their own: aero_kernel (dense arrays or per-vector records),
// aero_sm_kernel (spec-major records) and aero_wide_kernel (the rows the fused kernel's lanes do not reach), all three aero_body
// (gel_aero_body.h), with launch_aero and launch_aero_wide.
#include "gel_aero_body.h"

namespace gel {

constexpr int kAeroMinWaves = 3;   // waves/SIMD of aero_kernel and aero_sm_kernel (164 VGPRs)
// Workgroup p runs on XCD p % 8: in dispatch order every XCD works on every eighth run of entries, i.e. on every page of x and of the
// outputs that is in flight.  The workgroup index is permuted so that XCD j takes a contiguous eighth of the launch (as the fused
// kernel's vector groups, gel_eval_kernel.h); the workgroups behind the last multiple of eight keep their place.
__device__ __forceinline__ unsigned aero_xcd_block(unsigned p, unsigned n) {
  const unsigned n8 = n >> 3;
  return (p < 8u * n8) ? (p & 7u) * n8 + (p >> 3) : p;
}
__global__ __launch_bounds__(64 * kAeroWaves, kAeroMinWaves) void aero_kernel(ProblemDev P, int nnodes, const AeroNodeDev* __restrict__ nodes,
                                                                int tiles, int B, const double* __restrict__ x, AeroOut O) {
  aero_body<false>(P, nnodes, nodes, tiles, B, x, O, aero_xcd_block(blockIdx.x, gridDim.x));
}
__global__ __launch_bounds__(64 * kAeroWaves, kAeroMinWaves) void aero_sm_kernel(ProblemDev P, int nnodes, const AeroNodeDev* __restrict__ nodes,
                                                                   int tiles, int B, const double* __restrict__ x, AeroOut O) {
  aero_body<false, false, true>(P, nnodes, nodes, tiles, B, x, O, aero_xcd_block(blockIdx.x, gridDim.x));
}
__global__ __launch_bounds__(64 * kAeroWaves, 2) void aero_wide_kernel(ProblemDev P, int nnodes, const AeroNodeDev* __restrict__ nodes,
                                                                int B, const double* __restrict__ x, AeroOut O) {
  aero_body<false, true>(P, nnodes, nodes, 0, B, x, O, blockIdx.x);
}

// the listed nodes' rows into per-vector records: out.con / out.jac point at each kind's part of record 0, ld doubles per record
hipError_t launch_aero_wide(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                            const AeroLaunchOut& out, long long ld, hipStream_t s) {
  if (B <= 0 || nnodes <= 0) return hipSuccess;
  AeroOut O;
  for (int k = 0; k < 3; k++) { O.con[k] = out.con[k]; O.jac[k] = out.jac[k]; O.nrows[k] = out.nrows[k]; }
  O.ld = ld; O.sm = 0;
  const size_t lds = aero_lds_bytes(P.Kw, P.Kc);
  const long long waves = ((long long)B * nnodes + 63) / 64;
  hipLaunchKernelGGL(aero_wide_kernel, dim3((unsigned)((waves + kAeroWaves - 1) / kAeroWaves)), dim3(64 * kAeroWaves), lds, s, P, nnodes, nodes, B, d_x, O);
  return hipGetLastError();
}

// ld != 0: per-vector records (see AeroOut).  The flat mapping addresses a batch's gradient values with 32-bit byte offsets: a
// batch whose records span more is launched in runs of vectors that do not.
hipError_t launch_aero(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                       const AeroLaunchOut& out, hipStream_t s, long long ld, bool spec_major) {
  if (B <= 0 || nnodes <= 0) return hipSuccess;
  const AeroForm form = aero_form(nnodes, B, out.nrows, ld);
  if (form.runs > 1) {
    for (long long b0 = 0; b0 < B; b0 += form.run_len) {   // every run decides its own form: a last run of one vector takes a tile
      AeroLaunchOut o = out;
      for (int k = 0; k < 3; k++) { if (o.con[k]) o.con[k] += b0 * ld; if (o.jac[k]) o.jac[k] += b0 * ld; }
      const hipError_t e = launch_aero(P, nnodes, nodes, (int)std::min<long long>(form.run_len, B - b0), d_x + b0 * P.nvars, o, s, ld, spec_major);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  AeroOut O;
  for (int k = 0; k < 3; k++) { O.con[k] = out.con[k]; O.jac[k] = out.jac[k]; O.nrows[k] = out.nrows[k]; }
  O.ld = ld; O.sm = (ld > 0 && spec_major) ? 1 : 0;
  int tiles = (nnodes + 63) / 64;
  const size_t lds = aero_lds_bytes(P.Kw, P.Kc);
  long long waves = (long long)B * tiles;
  // flat (vector, node) mapping (tiles = 0 tells the kernel): no mostly-empty last tile per vector; needs every wavefront inside two
  // vectors and the batch's gradient values of a kind inside 32-bit byte offsets
  if (form.flat) {
    waves = ((long long)B * nnodes + 63) / 64;
    tiles = 0;
  }
  const unsigned grid = (unsigned)((waves + kAeroWaves - 1) / kAeroWaves);
  if (O.sm) hipLaunchKernelGGL(aero_sm_kernel, dim3(grid), dim3(64 * kAeroWaves), lds, s, P, nnodes, nodes, tiles, B, d_x, O);
  else hipLaunchKernelGGL(aero_kernel, dim3(grid), dim3(64 * kAeroWaves), lds, s, P, nnodes, nodes, tiles, B, d_x, O);
  return hipGetLastError();
}

}  // namespace gel
