// gel_launch.h -- host-callable launchers of the evaluation path's kernels; each group names the file that defines it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gel_device.h"

namespace gel {

// the form of the fused kernel a launch takes: <JAC, MFMA, SPLIT, PACK> and its wavefront count
// (gel_kernels.hip)
struct EvalForm { bool jac, mfma, split, pack; long long waves; };
EvalForm eval_form(const ProblemDev& P, int B, bool want_res, bool want_jac);
hipError_t launch_eval(const ProblemDev& P, int B, const double* d_x, double* d_res, double* d_jvar, hipStream_t s);
// grid of a cooperative launch of the fused kernel, vw decision vectors per workgroup: the vector-group major order deals the groups
// to the eight XCDs in blocks of eight (short last block: idle workgroups leave at once)
inline unsigned coop_grid(const ProblemDev& P, int B, int vw) {
  const unsigned nb = (unsigned)((B + vw - 1) / vw);
  return P.vmajor ? (unsigned)P.nchunks * 8u * ((nb + 7u) / 8u) : (unsigned)P.nchunks * nb;
}
// defect groups + the aero rows of the aerodynamic phases' nodes 1 .. n in ONE launch (gel_kernels_aero.hip: the AERO instantiation)
bool eval_aero_fusable(const ProblemDev& P, int B);
hipError_t launch_eval_aero(const ProblemDev& P, int B, const double* d_x, double* d_res, double* d_jvar, hipStream_t s);
// exact Jacobian of the defect groups (gel_kernels_exact.hip, GEL_FLAG_EXACT_DEFECT_JAC): the compact values only, no residuals
hipError_t launch_eval_exact(const ProblemDev& P, int B, const double* d_x, double* d_jvar, hipStream_t s);
// the full COO value buffers (gel_kernels_coo.hip)
hipError_t launch_expand(long long nnz, long long V, int B, const double* cval, const int32_t* src,
                         const double* d_jvar, double* d_full, hipStream_t s);
// x-dependent entries only, into a full COO buffer that holds the constants (launch_fill_full lays them down)
hipError_t launch_update_full(long long nnz, long long V, int nvar, int B, const int32_t* vdst, const int32_t* vsrc,
                              int nlines, const int32_t* vline, const int32_t* src, const double* cval,
                              const double* d_jvar, double* d_full, hipStream_t s);
hipError_t launch_fill_full(long long nnz, int B, const double* cval, double* d_full, hipStream_t s);
// packed unit-shard exchange buffer [nranks][B][width] -> the ordinary res [B][nres] / jvar [B][V] layouts (either may be null)
hipError_t launch_shard_unpack(long long nres, long long V, long long width, int B, const int64_t* pos, const double* out,
                               double* d_res, double* d_jvar, hipStream_t s);
// the generic forward difference (gel_kernels_fd.hip)
hipError_t launch_perturb_local(int nloc, double dx, const double* d_x, const int32_t* d_colmap, double* d_Xp, hipStream_t s);
hipError_t launch_quotient_local(int nloc, int nres, int roff, int nrows, double dx, const double* d_res, double* d_J,
                                 long long ldJ, int row0, const int32_t* d_colmap, hipStream_t s);
// the RHS and point test hooks (gel_kernels_hooks.hip)
hipError_t launch_rhs_vel(bool air, int n, const double* mass_e, const double* pos_e, const double* vel_e,
                          const double* quat, const double* t, const double* tables, int Kw, int Kc, double thrust,
                          double area, double nozzle, double um, double up, double uv, double barC20, double* out,
                          hipStream_t s);
hipError_t launch_rhs_quat(int n, const double* quat, const double* u_e, double unit_u, double* out, hipStream_t s);
hipError_t launch_point(int kind, int n, const double* in, const double* aux, int aux_rows, double* out,
                        hipStream_t s);

// the aero rows on their own (gel_kernels_aerorows.hip)
// outputs of one aero launch: per kind (0 alpha, 1 q, 2 q-alpha) the constraint vector and the COO values, or null
struct AeroLaunchOut { double* con[3]; double* jac[3]; int32_t nrows[3]; };
// the form a launch_aero of B vectors takes: flat (vector, node) mapping or one tile per vector (of a full-length run), the runs
// the batch is launched in and their length in vectors, and the bytes one launch's gradient values of the largest kind span
// (what the flat mapping addresses with 32-bit byte offsets)
struct AeroForm { bool flat; long long runs, run_len, max_bytes; };
// The decision at the top of launch_aero (host only; also reported through gel_aero_launch_info).  The flat (vector, node) mapping
// needs every wavefront inside two vectors (nnodes >= 64, not a multiple of 64, more than one vector) and the gradient values of a
// kind inside 32-bit byte offsets: dense arrays (ld = 0) beyond 2^32 - 2^24 bytes take one tile per vector instead; a batch of
// records (ld != 0) whose span exceeds 2^32 - 2^25 bytes is launched in runs of vectors that stay below it.
inline AeroForm aero_form(int nnodes, int B, const int32_t* nrows, long long ld) {
  AeroForm f{false, 1, B, 0};
  if (B <= 0 || nnodes <= 0) return f;
  const bool flat_shape = B > 1 && nnodes >= 64 && (nnodes & 63) != 0;
  if (ld > 0 && flat_shape) {
    const long long run = ((1LL << 32) - (1LL << 25)) / (ld * 8);
    if (run >= 1 && run < B) { f.runs = (B + run - 1) / run; f.run_len = run; }
  }
  for (int k = 0; k < 3; k++) f.max_bytes = std::max(f.max_bytes, f.run_len * (ld ? ld : (long long)nrows[k] * (8 + ((k == 1) ? 0 : 4))) * 8);
  f.flat = f.run_len > 1 && nnodes >= 64 && (nnodes & 63) != 0 && f.max_bytes < (1LL << 32) - (1LL << 24);
  return f;
}
hipError_t launch_aero(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                       const AeroLaunchOut& out, hipStream_t s, long long ld = 0, bool spec_major = false);

// exact gradients of the aero kinds (gel_kernels_exact_aero.hip, GEL_FLAG_EXACT_AERO_JAC): out.jac only, in launch_aero's addressing
// (ld = 0 dense arrays; ld != 0 records, spec_major part A or part B); the values come from a launch_aero without gradient outputs
hipError_t launch_aero_exact(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                             const AeroLaunchOut& out, hipStream_t s, long long ld = 0, bool spec_major = false);

hipError_t launch_aero_wide(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                            const AeroLaunchOut& out, long long ld, hipStream_t s);

// (gel_kernels.hip) one callback = one launch: defect groups (split form) + aero kinds + row table as workgroup ranges of one grid; aero / d_con
// may be null (that part is left out)
hipError_t launch_callback(const ProblemDev& P, bool want_jac, const double* d_x, double* d_res, double* d_jvar,
                           int nnodes, const AeroNodeDev* nodes, const AeroLaunchOut* aero,
                           int nlin, const LinRowDev* lin, int nfn, const FnRowDev* fr, double* d_con, double* d_jfn, hipStream_t s);
// the row table and the post-processing table (gel_kernels_rows.hip)
hipError_t launch_rows(const ProblemDev& P, int nlin, const LinRowDev* lin, int nfn, const FnRowDev* fr, int B,
                       const double* d_x, double* d_con, double* d_jfn, hipStream_t s);
// exact Jacobian of the node-function rows (gel_kernels_exact_rows.hip, GEL_FLAG_EXACT_ROWS_JAC): jfn [B][nfn][7] only, in
// launch_rows' layout; the values come from a launch_rows without a jfn output
hipError_t launch_rows_exact(const ProblemDev& P, int nfn, const FnRowDev* fr, int B, const double* d_x, double* d_jfn, hipStream_t s);

// post-processing table (output_result.py): kOutputColumns values per state node, see include/gelato_amd.h
constexpr int kOutputColumns = 34;
hipError_t launch_output(const ProblemDev& P, int M, const double* d_x, const double* d_tx, const int32_t* d_node_sec,
                         double lat0, double lon0, double* d_out, hipStream_t s);

// US-1976 layer table as the kernels expect it: Lmb[11] | Tmb[11] | Pb[11] | R[11] | pexp[11] | gR[11] | Hb[11] | 1/Tmb[11]
constexpr int kAtmTableDoubles = 88;  // must equal kAtmDoubles of gel_physics.h (static_assert in gel_tables.h)
void fill_atmosphere_table(double* atm);
const char* check_tables(const double* wind, int Kw, const double* ca, int Kc);
std::vector<double> build_tables(const double* wind, int Kw, const double* ca, int Kc);
void append_rows_and_slopes(std::vector<double>& rows_out, std::vector<double>& slopes_out, const double* tab, int K, int w);
// doubles of the staged tables (atmosphere | wind rows | CA rows | wind slopes | CA slopes), as gel_physics.h table_doubles()
inline size_t staged_table_doubles(int Kw, int Kc) { return (size_t)kAtmTableDoubles + 3 * (size_t)Kw + 2 * (size_t)Kc + 2 * (size_t)(Kw - 1) + (size_t)(Kc - 1); }

// LDS of the launches that stage the tables.  They pass no launch attribute, so a workgroup may take kLaunchMaxLds bytes at most;
// the launchers size their launches with these functions and the host refuses with them (gel_host.hip: gel_problem_create,
// gel_mesh_error, gel_dynamics_velocity, gel_point_eval; gel_table_limits reports them) before anything is enqueued.
constexpr size_t kLaunchMaxLds = 64 * 1024;
// first double behind the staged tables (ProblemDev::park_off; the park base of aero_body, `base` of mesh_kernel): kept even
inline size_t padded_table_doubles(int Kw, int Kc) { return (staged_table_doubles(Kw, Kc) + 1) & ~(size_t)1; }
inline size_t table_lds_bytes(int Kw, int Kc) { return sizeof(double) * staged_table_doubles(Kw, Kc); }   // the kernels that keep nothing behind the tables
size_t eval_lds_bytes_max(int Kw, int Kc);   // the fused kernel's largest form (gel_kernels.hip)
size_t aero_lds_bytes(int Kw, int Kc);       // (gel_kernels.hip) aero_kernel, aero_sm_kernel, aero_wide_kernel; callback_kernel takes the larger of the two
inline size_t point_lds_bytes(int aux_rows) { return sizeof(double) * (size_t)(kAtmTableDoubles + 5 * (aux_rows > 0 ? aux_rows : 0)); }

}  // namespace gel
