// gel_kernels.hip -- the fused evaluation kernel's launches (eval_kernel and eval_body: gel_eval_kernel.h) and the one-launch
// callback.
//   eval_form / launch_eval   which instantiation a launch takes, and the launch: the cooperative forms (launch_coop), the split
//                             latency form, the wavefront dot-product forms
//   callback_kernel           ONE launch for one callback of the optimiser: eval_body (split form), aero_body (gel_aero_body.h)
//                             and rows_body (gel_rows_body.h) as workgroup ranges of one grid; launch_callback
//   eval_lds_bytes_max, aero_lds_bytes   the LDS of those launches (the host refuses tables that do not fit before anything is enqueued)
// The AERO instantiation of eval_kernel is gel_kernels_aero.hip (its own scheduling strategy); the other kernels of the evaluation
// path are gel_kernels_aerorows.hip, gel_kernels_rows.hip, gel_kernels_coo.hip, gel_kernels_fd.hip and gel_kernels_hooks.hip.
//
// Data layout (HBM):
//   x     [B][nvars]  packed xdict (AoS per node, as the boundary hands it over)
//   res   [B][11N]    mass N | pos 3N | vel 3N | quat 4N
//   jvar  [B][V]      per phase [slot][node]: consecutive lanes (nodes) write
//                     consecutive doubles -> every store instruction is one
//                     contiguous 512-byte segment per wavefront.
//   Dt    per phase, transposed (Dt[i*n + j] = D[j][i]) so lane j reads
//         consecutive addresses while all lanes share X[i][c] (broadcast).
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_aero_body.h"
#include "gel_rows_body.h"

#include "gel_eval_kernel.h"
namespace gel {

// every form's region per wavefront fits the Jacobian forms' park, so eval_lds_bytes_max() bounds every launch of the fused kernel
static_assert(wave_lds_doubles(false, false, false) <= kWaveLds && wave_lds_doubles(false, true, false, true) <= kWaveLds &&
              wave_lds_doubles(false, true, true) <= kWaveLds && wave_lds_doubles(false, true, false, false, true) <= kWaveLds &&
              wave_lds_doubles(false, true, false, false, false) <= kWaveLds, "kWaveLds is the largest region");
static size_t eval_lds_bytes(size_t park_off, int wave_doubles) { return sizeof(double) * (park_off + (size_t)wave_doubles * (kBlock / 64)); }
size_t eval_lds_bytes_max(int Kw, int Kc) { return eval_lds_bytes(padded_table_doubles(Kw, Kc), kWaveLds); }
size_t aero_lds_bytes(int Kw, int Kc) { return sizeof(double) * (padded_table_doubles(Kw, Kc) + (size_t)kAeroWaves * kAeroParkSlots * 64); }

// launches with at most this many wavefronts (after the x4) use the split latency form: one per SIMD
constexpr long long kSplitMaxWaves = 1024;

// which instantiation a launch takes (also reported through gel_launch_info)
EvalForm eval_form(const ProblemDev& P, int B, bool want_res, bool want_jac) {
  EvalForm f;
  const long long waves = (long long)B * P.nchunks;
  f.jac = want_jac;
  // D.X on the matrix pipe only when residual rows are requested at all and the problem asks for it
  f.mfma = P.use_mfma && want_res;
  // a handful of vectors cannot fill 1024 SIMDs: trade recomputation of the centre for a shorter serial chain;
  // P.nunits > 0: the caller asked for a range of units (unit-sharded launch)
  f.split = want_jac && (P.nunits > 0 || waves * 4 <= kSplitMaxWaves);
  // two decision vectors per wavefront: cooperative form (matrix pipe, not split) of a problem whose phases all fit 32 lanes
  f.pack = f.mfma && !f.split && P.pack;
  const int vw = f.pack ? 8 : 4;   // decision vectors per workgroup of the cooperative form
  f.waves = f.split ? (long long)B * (P.nunits > 0 ? P.nunits : 4 * P.nchunks)
                    : (f.mfma ? 4LL * P.nchunks * ((B + vw - 1) / vw) : waves);
  return f;
}

template <bool JAC, bool PACK, bool LONGP, bool NTS = true>
static void launch_coop(const ProblemDev& P, int B, const double* d_x, double* d_res, double* d_jvar, hipStream_t s) {
  const unsigned grid = coop_grid(P, B, PACK ? 8 : 4);
  const size_t lds = eval_lds_bytes((size_t)P.park_off, wave_lds_doubles(JAC, true, PACK, false, LONGP));
  hipLaunchKernelGGL((eval_kernel<JAC, true, false, PACK, LONGP, NTS>), dim3(grid), dim3(kBlock), lds, s, P, B, d_x, d_res, d_jvar);
}

hipError_t launch_eval(const ProblemDev& P, int B, const double* d_x, double* d_res, double* d_jvar, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const EvalForm f = eval_form(P, B, d_res != nullptr, d_jvar != nullptr);
  if (f.mfma && !f.split) {
    // cooperative D.X form (matrix pipe, not split): one workgroup = one work item x four (PACK: eight) decision vectors
    // Jacobian values of a launch that fits the Infinity Cache (256 MB) and is read again at once (gel_eval_full_device: the update of
    // a full COO buffer) by ordinary stores: the reader finds them there (fused + update at B = 1024: 0.26 -> 0.165 ms).  A launch on
    // its own is better off streaming them past the caches even when it is small (B = 256 on repeat: ordinary stores +9 %)
    const bool small = P.cached_out && (double)B * 8.0 * ((double)P.V + 11.0 * P.N) <= 192.0e6;
    if (f.jac && f.pack) { if (small) launch_coop<true, true, false, false>(P, B, d_x, d_res, d_jvar, s); else launch_coop<true, true, false, true>(P, B, d_x, d_res, d_jvar, s); }
    // one Jacobian instantiation for long and short phases (without the slab loop it measured 0.4 % SLOWER at 6 x 64, with 52
    // fewer instructions per wavefront); the residual-only form of a problem without a long phase drops to 72 VGPRs without it
    // (7 waves/SIMD: -10 % launch time at 6 x 64)
    else if (f.jac) { if (small) launch_coop<true, false, true, false>(P, B, d_x, d_res, d_jvar, s); else launch_coop<true, false, true, true>(P, B, d_x, d_res, d_jvar, s); }
    else if (f.pack) launch_coop<false, true, false>(P, B, d_x, d_res, d_jvar, s);
    else if (P.longp) launch_coop<false, false, true>(P, B, d_x, d_res, d_jvar, s);
    else launch_coop<false, false, false>(P, B, d_x, d_res, d_jvar, s);
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((f.waves * 64 + kBlock - 1) / kBlock);
  // tables | one region per wavefront (the park, or only what a residual-only launch parks)
  const size_t lds = eval_lds_bytes((size_t)P.park_off, wave_lds_doubles(f.jac, f.mfma, false));
  if (f.split) {
    ProblemDev Q = P;
    if (Q.nunits <= 0) { Q.unit0 = 4 * P.chunk0; Q.nunits = 4 * P.nchunks; }  // the whole list, split
    if (Q.done_flag) Q.done_total = (int32_t)grid;
    if (f.mfma)
      hipLaunchKernelGGL((eval_kernel<true, true, true>), dim3(grid), dim3(kBlock), lds, s, Q, B, d_x, d_res, d_jvar);
    else
      hipLaunchKernelGGL((eval_kernel<true, false, true>), dim3(grid), dim3(kBlock), lds, s, Q, B, d_x, d_res, d_jvar);
    return hipGetLastError();
  }
  if (f.jac)
    hipLaunchKernelGGL((eval_kernel<true, false>), dim3(grid), dim3(kBlock), lds, s, P, B, d_x, d_res, d_jvar);
  else
    hipLaunchKernelGGL((eval_kernel<false, false>), dim3(grid), dim3(kBlock), lds, s, P, B, d_x, d_res, d_jvar);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ONE launch for one callback of the optimiser (Trajectory_Optimization.py:194-312 at B = 1): the four defect groups in the
// split latency form (its own wavefronts, one unit each), the aero path constraints and the row table, as workgroup
// ranges of the same grid -- nothing waits for anything, so the three run side by side instead of one launch after the
// other (three launches on one stream: 30 us of kernels back to back + two more launch latencies; three streams cost
// more than they saved: 94 us against 65).  Same device functions, same bits as the separate launches.
// 256 threads: the aero workgroup (one wavefront per sweep role) and four units of the split form.
// ---------------------------------------------------------------------------
struct CallbackArgs {
  int32_t nb_eval, nb_aero;
  int32_t nnodes, tiles;
  const AeroNodeDev* nodes;
  AeroOut O;
  int32_t nlin, nfn, lin_blocks;
  const LinRowDev* lin;
  const FnRowDev* fr;
  double* con;
  double* jfn;
};
static_assert(64 * kAeroWaves == 256, "callback_kernel's workgroup is the aero workgroup (four roles of one tile)");
template <bool JAC, bool MFMA>
__global__ __launch_bounds__(256) void callback_kernel(ProblemDev P, const double* __restrict__ x, double* __restrict__ res,
                                                       double* __restrict__ jvar, CallbackArgs A) {
  const unsigned b = blockIdx.x;
  if (b < (unsigned)A.nb_eval) eval_body<JAC, MFMA, true, false, 17>(P, 1, x, res, jvar, b);
  else if (b < (unsigned)(A.nb_eval + A.nb_aero)) aero_body<true>(P, A.nnodes, A.nodes, A.tiles, 1, x, A.O, b - (unsigned)A.nb_eval);
  else rows_body(P, A.nlin, A.lin, A.nfn, A.fr, 1, A.lin_blocks, x, A.con, A.jfn, b - (unsigned)(A.nb_eval + A.nb_aero));
  signal_done(P);
}

hipError_t launch_callback(const ProblemDev& P0, bool want_jac, const double* d_x, double* d_res, double* d_jvar,
                           int nnodes, const AeroNodeDev* nodes, const AeroLaunchOut* aero,
                           int nlin, const LinRowDev* lin, int nfn, const FnRowDev* fr, double* d_con, double* d_jfn, hipStream_t s) {
  ProblemDev P = P0;
  P.unit0 = 4 * P0.chunk0;
  P.nunits = 4 * P0.nchunks;                       // every unit of the problem, split form
  CallbackArgs A{};
  A.nb_eval = (P.nunits + 3) / 4;                  // four wavefronts = four units per workgroup
  if (aero && nnodes > 0) {
    for (int k = 0; k < 3; k++) { A.O.con[k] = aero->con[k]; A.O.jac[k] = aero->jac[k]; A.O.nrows[k] = aero->nrows[k]; }
    A.O.ld = 0; A.O.sm = 0;
    A.nnodes = nnodes; A.nodes = nodes; A.tiles = (nnodes + 63) / 64; A.nb_aero = A.tiles;   // ROLES form: one workgroup per tile
  }
  int rows_blocks = 0;
  if (d_con && nlin + nfn > 0) {
    A.nlin = nlin; A.nfn = nfn; A.lin = lin; A.fr = fr; A.con = d_con; A.jfn = d_jfn;
    A.lin_blocks = (nlin + 255) / 256;
    rows_blocks = A.lin_blocks + (nfn * 8 + 255) / 256;
  }
  const size_t lds_eval = eval_lds_bytes((size_t)P.park_off, wave_lds_doubles(want_jac, P.use_mfma != 0, false, true));
  const size_t lds_aero = aero_lds_bytes(P.Kw, P.Kc);
  const size_t lds = lds_eval > lds_aero ? lds_eval : lds_aero;
  const dim3 grid((unsigned)(A.nb_eval + A.nb_aero + rows_blocks));
  if (P.done_flag) P.done_total = (int32_t)grid.x;
  if (want_jac) {
    if (P.use_mfma) hipLaunchKernelGGL((callback_kernel<true, true>), grid, dim3(256), lds, s, P, d_x, d_res, d_jvar, A);
    else hipLaunchKernelGGL((callback_kernel<true, false>), grid, dim3(256), lds, s, P, d_x, d_res, d_jvar, A);
  } else {
    if (P.use_mfma) hipLaunchKernelGGL((callback_kernel<false, true>), grid, dim3(256), lds, s, P, d_x, d_res, d_jvar, A);
    else hipLaunchKernelGGL((callback_kernel<false, false>), grid, dim3(256), lds, s, P, d_x, d_res, d_jvar, A);
  }
  return hipGetLastError();
}

}  // namespace gel
