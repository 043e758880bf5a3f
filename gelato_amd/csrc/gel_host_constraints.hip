// gel_host_constraints.hip -- every constraint that is not a defect row: the point-dynamics entries, the aero path
// constraints (gel_aero_*, gel_eval_*aero*; 3.4, 3.7), the knot / terminal / user rows (gel_rows_*; 3.5, 3.8) and the products with
// their Jacobian K (gel_con_*; 3.15).  One file: conprod_build makes K's tables for gel_aero_configure and gel_rows_configure alike.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "gel_host_handle.h"

using namespace gelhost;

namespace {
constexpr const char* kNoGpuConprod = "host-only handle: the device products need a GPU (gel_con_products_host runs on the host)";
}  // namespace

extern "C" {

// --------------------------- RHS / point hooks ---------------------------
int gel_dynamics_velocity(int32_t n, const double* mass_e, const double* pos_e, const double* vel_e, const double* quat,
                          const double* t, const double* param, const double* wind, int32_t Kw, const double* ca,
                          int32_t Kc, const double* units, double barC20, double* out) {
  if (n < 0 || !mass_e || !pos_e || !vel_e || !quat || !t || !param || !wind || !ca || !units || !out)
    return fail(GEL_ERR_ARG, "null argument");
  if (n == 0) return GEL_OK;
  if (Kw < 2 || Kc < 2) return fail(GEL_ERR_ARG, "the wind and CA tables need at least two rows");
  int rc = check_launch_lds("gel_dynamics_velocity", gel::table_lds_bytes(Kw, Kc), gel::staged_table_doubles(Kw, Kc), gel::staged_table_doubles(Kw, Kc), false);
  if (rc) return rc;
  rc = need_device();
  if (rc) return rc;
  if (const char* why = gel::check_tables(wind, Kw, ca, Kc)) return fail(GEL_ERR_ARG, why);
  const std::vector<double> tables = gel::build_tables(wind, Kw, ca, Kc);
  DeviceArray<double> m, r, v, q, tt, tb, o;
  HIPCHK(m.upload(mass_e, n)); HIPCHK(r.upload(pos_e, 3 * (size_t)n)); HIPCHK(v.upload(vel_e, 3 * (size_t)n));
  HIPCHK(q.upload(quat, 4 * (size_t)n)); HIPCHK(tt.upload(t, n)); HIPCHK(tb.upload(tables)); HIPCHK(o.reserve(3 * (size_t)n));
  if (barC20 == 0.0) barC20 = -0.484165371736e-3;
  HIPCHK(gel::launch_rhs_vel(true, n, m.get(), r.get(), v.get(), q.get(), tt.get(), tb.get(), Kw, Kc, param[0], param[2], param[4],
                             units[0], units[1], units[2], barC20, o.get(), nullptr));
  HIPCHK(hipMemcpy(out, o.get(), 3 * (size_t)n * 8, hipMemcpyDeviceToHost));
  return GEL_OK;
}

int gel_dynamics_velocity_NoAir(int32_t n, const double* mass_e, const double* pos_e, const double* quat,
                                const double* param, const double* units, double barC20, double* out) {
  if (n < 0 || !mass_e || !pos_e || !quat || !param || !units || !out) return fail(GEL_ERR_ARG, "null argument");
  if (n == 0) return GEL_OK;
  int rc = need_device();
  if (rc) return rc;
  DeviceArray<double> m, r, q, o;
  HIPCHK(m.upload(mass_e, n)); HIPCHK(r.upload(pos_e, 3 * (size_t)n)); HIPCHK(q.upload(quat, 4 * (size_t)n)); HIPCHK(o.reserve(3 * (size_t)n));
  if (barC20 == 0.0) barC20 = -0.484165371736e-3;
  HIPCHK(gel::launch_rhs_vel(false, n, m.get(), r.get(), nullptr, q.get(), nullptr, nullptr, 0, 0, param[0], 0.0, 0.0, units[0],
                             units[1], units[2], barC20, o.get(), nullptr));
  HIPCHK(hipMemcpy(out, o.get(), 3 * (size_t)n * 8, hipMemcpyDeviceToHost));
  return GEL_OK;
}

int gel_dynamics_quaternion(int32_t n, const double* quat, const double* u_e, double unit_u, double* out) {
  if (n < 0 || !quat || !u_e || !out) return fail(GEL_ERR_ARG, "null argument");
  if (n == 0) return GEL_OK;
  int rc = need_device();
  if (rc) return rc;
  DeviceArray<double> q, u, o;
  HIPCHK(q.upload(quat, 4 * (size_t)n)); HIPCHK(u.upload(u_e, 2 * (size_t)n)); HIPCHK(o.reserve(4 * (size_t)n));
  HIPCHK(gel::launch_rhs_quat(n, q.get(), u.get(), unit_u, o.get(), nullptr));
  HIPCHK(hipMemcpy(out, o.get(), 4 * (size_t)n * 8, hipMemcpyDeviceToHost));
  return GEL_OK;
}

// The two walks that describe the aero gradients of a configuration `a` of handle p (gel_aero_pattern, gel_aero_record_map and
// the tables of the K products all go through them: there is no second description of the layout).
// emission order of inequality_jac_max_*: con_aero.py:437-463
static void aero_pattern_of(const gel_problem* p, const gel_problem::Aero& a, int kind, int var, int32_t* rows, int32_t* cols) {
  const auto& A = a.rows[kind];
  int64_t o = 0;
  for (size_t r0 = 0; r0 < A.size(); r0 += A[r0].nk) {
    const int nk = A[r0].nk, i = A[r0].phase, xa = p->ph[i].xa, iRow = (int)r0;
    if (var == 3) {
      for (int k = 0; k < nk; k++) { rows[o] = iRow + k; cols[o++] = i; }
      for (int k = 0; k < nk; k++) { rows[o] = iRow + k; cols[o++] = i + 1; }
    } else if (!(var == 2 && kind == 1)) {
      const int w = (var == 2) ? 4 : 3;
      for (int j = 0; j < w; j++)
        for (int k = 0; k < nk; k++) { rows[o] = iRow + k; cols[o++] = (xa + k) * w + j; }
    }
  }
}
// record index of every entry of gel_eval_aero_all's arrays: var = -1 the constraint vector [nrows], var 0..3 the position /
// velocity / quaternion / t block of the gradient values (in the order of aero_pattern_of)
static void aero_record_map_of(const gel_problem* p, const gel_problem::Aero& a, int kind, int var, int64_t* idx) {
  const auto& A = a.rows[kind];
  const int nq = (kind == 1) ? 0 : 4;
  int64_t o = 0;
  if (var == -1) {
    for (size_t r = 0; r < A.size(); r++) {
      const int32_t po = a.part_of[kind][r];
      if (po & 1) idx[o++] = a.off_con[1][kind] + (po >> 1);
      else idx[o++] = a.partA_base[kind][po >> 1] + ((po >> 1) - a.part_rows[0][kind][po >> 1].row0);
    }
    return;
  }
  if (var == 2 && kind == 1) return;   // dynamic pressure has no quaternion block
  const int64_t w = (var == 2) ? 4 : ((var == 3) ? 2 : 3);
  const int64_t bo = (var == 0) ? 0 : ((var == 1) ? 3 : ((var == 2) ? 6 : 6 + nq));
  for (size_t r0 = 0; r0 < A.size(); r0 += A[r0].nk)
    for (int64_t j = 0; j < w; j++)
      for (int k = 0; k < A[r0].nk; k++) {     // the reference's emission order: spec, column, node (aero_pattern_of)
        const int32_t po = a.part_of[kind][r0 + k];
        const int part = po & 1;
        const auto& q = a.part_rows[part][kind][po >> 1];
        const int64_t R = (int64_t)a.part_rows[part][kind].size();
        const int64_t ko = (po >> 1) - q.row0;
        if (part == 1) idx[o++] = a.off_jac[1][kind] + bo * R + w * q.row0 + j * q.nk + ko;
        else if (var == 3 && !p->fd_recompute) idx[o++] = -1;      // an exact zero, not stored (AeroPhaseDev)
        else idx[o++] = a.partA_base[kind][po >> 1] + (((var == 0) ? 1 : ((var == 1) ? 4 : ((var == 2) ? 7 : 11))) + j) * q.nk + ko;
      }
}

// The tables of the K products (gel_conprod.h) for the row table (lin, fn) and the aero configuration a, host arrays and device
// copies, into `out` (a local of the configure call that swaps it in).  Rows [linear | node-function | alpha | q | q-alpha];
// a row's entries in the order of its definition (linear: idx0, idx1; node-function: jfn column 0 .. 6; aero: var 0 .. 3, inside
// a var the pattern's order); a column's entries by ascending row, equal rows in the row's own order.
static int conprod_build(const gel_problem* p, const std::vector<gel::LinRowDev>& lin, const std::vector<gel::FnRowDev>& fn,
                  const gel_problem::Aero& a, gel_problem::Conprod& out) {
  struct Entry { int32_t row, col, src; int64_t offd, offr; double cval; };
  const int M = p->dims.M, N = p->dims.N, nvars = p->dims.num_vars;
  const int32_t var_off[4] = {M, 4 * M, 7 * M, 11 * M + 2 * N};   // position, velocity, quaternion, t inside the packed vector
  std::vector<std::vector<Entry>> by_row;
  out.nlin = (int32_t)lin.size(); out.nfn = (int32_t)fn.size();
  for (size_t r = 0; r < lin.size(); r++) {
    by_row.emplace_back();
    by_row.back().push_back(Entry{(int32_t)r, lin[r].idx0, gel::kConSrcConst, 0, 0, lin[r].coef0});
    if (lin[r].idx1 >= 0) by_row.back().push_back(Entry{(int32_t)r, lin[r].idx1, gel::kConSrcConst, 0, 0, lin[r].coef1});
  }
  for (size_t r = 0; r < fn.size(); r++) {
    by_row.emplace_back();
    const int32_t row = out.nlin + (int32_t)r;
    for (int c = 0; c < 6; c++)
      by_row.back().push_back(Entry{row, var_off[c / 3] + 3 * fn[r].node + c % 3, gel::kConSrcJfn, (int64_t)r * 7 + c, (int64_t)r * 7 + c, 0.0});
    if (fn[r].tcol >= 0)   // jfn[r][6] of a row without a time column is never read
      by_row.back().push_back(Entry{row, var_off[3] + fn[r].tcol, gel::kConSrcJfn, (int64_t)r * 7 + 6, (int64_t)r * 7 + 6, 0.0});
  }
  int32_t row0 = out.nlin + out.nfn;
  for (int kd = 0; kd < 3; kd++) {
    const int64_t Rk = (int64_t)a.rows[kd].size();
    out.nrows[kd] = (int32_t)Rk;
    out.jac_len[kd] = Rk * ((kd == 1) ? 8 : 12);
    by_row.resize((size_t)row0 + Rk);
    int64_t dense0 = 0;
    for (int var = 0; var < 4; var++) {
      const int64_t nnz = (var == 3) ? 2 * Rk : ((var == 2) ? ((kd == 1) ? 0 : 4 * Rk) : 3 * Rk);
      std::vector<int32_t> rows(nnz), cols(nnz);
      std::vector<int64_t> rec(nnz);
      if (nnz) { aero_pattern_of(p, a, kd, var, rows.data(), cols.data()); aero_record_map_of(p, a, kd, var, rec.data()); }
      for (int64_t e = 0; e < nnz; e++)
        if (rec[e] >= 0)   // a structural zero is not an entry of K, in either source form
          by_row[(size_t)row0 + rows[e]].push_back(Entry{row0 + rows[e], var_off[var] + cols[e], gel::kConSrcAero0 + kd, dense0 + e, rec[e], 0.0});
      dense0 += nnz;
    }
    row0 += (int32_t)Rk;
  }
  out.R = row0;
  std::vector<Entry> all;
  for (const auto& r : by_row) all.insert(all.end(), r.begin(), r.end());
  if (all.size() > (size_t)0x7fffffff) return fail(GEL_ERR_ARG, "K products: too many entries");
  out.nnz = (int64_t)all.size();
  out.max_row = out.max_col = 0;
  for (int d = 0; d < 2; d++) {
    gel_problem::Conprod::Dir& D = out.dir[d];
    const int nout = d ? nvars : (int)out.R;
    if (d) std::stable_sort(all.begin(), all.end(), [](const Entry& x, const Entry& y) { return x.col < y.col; });
    D.ptr.assign((size_t)nout + 1, 0);
    for (const Entry& e : all) D.ptr[(size_t)(d ? e.col : e.row) + 1]++;
    for (int o = 0; o < nout; o++) {
      (d ? out.max_col : out.max_row) = std::max<int64_t>(d ? out.max_col : out.max_row, D.ptr[(size_t)o + 1]);
      D.ptr[(size_t)o + 1] += D.ptr[o];
    }
    D.idx.clear(); D.src.clear(); D.offd.clear(); D.offr.clear(); D.cval.clear();
    for (const Entry& e : all) {
      D.idx.push_back(d ? e.row : e.col); D.src.push_back(e.src); D.offd.push_back(e.offd); D.offr.push_back(e.offr);
      D.cval.push_back(e.cval);
    }
    if (p->device != GEL_DEVICE_NONE) {
      HIPCHK(D.d_ptr.upload(D.ptr)); HIPCHK(D.d_idx.upload(D.idx)); HIPCHK(D.d_src.upload(D.src));
      HIPCHK(D.d_offd.upload(D.offd)); HIPCHK(D.d_offr.upload(D.offr)); HIPCHK(D.d_cval.upload(D.cval));
    }
  }
  return GEL_OK;
}

// ------------------ aero path constraints (lib/con_aero.py) ------------------
int gel_aero_configure(gel_problem* p, int32_t kind, int32_t nspec, const int32_t* phase, const int32_t* range_all,
                       const double* limit) {
  if (!p || kind < 0 || kind > 2 || nspec < 0 || (nspec && (!phase || !range_all || !limit)))
    return fail(GEL_ERR_ARG, "bad argument");
  std::vector<gel::AeroRowDev> rows;
  int prev = -1;
  for (int s = 0; s < nspec; s++) {
    // the reference walks range(num_sections - 1) in order (con_aero.py:108): the last phase is never constrained
    if (phase[s] < 0 || phase[s] >= (int)p->ph.size() - 1 || phase[s] <= prev)
      return fail(GEL_ERR_ARG, "aero specs must name increasing phases in [0, num_sections - 1)");
    if (!(limit[s] != 0.0)) return fail(GEL_ERR_ARG, "aero limit must be non-zero");
    prev = phase[s];
    const int nk = range_all[s] ? p->ph[phase[s]].n + 1 : 1;
    const int row0 = (int)rows.size();
    for (int k = 0; k < nk; k++) rows.push_back(gel::AeroRowDev{phase[s], k, nk, row0, limit[s]});
  }
  // the whole new configuration in a local, swapped in only once everything has succeeded: a failed call leaves the old one in
  // place, on the host and on the device
  gel_problem::Aero a;
  for (int kd = 0; kd < 3; kd++) a.rows[kd] = (kd == kind) ? rows : p->aero.rows[kd];
  // the union of the constrained state nodes over the three kinds, in (phase, node) order
  for (int i = 0; i + 1 < (int)p->ph.size(); i++)
    for (int k = 0; k <= p->ph[i].n; k++) {
      gel::AeroNodeDev nd{i, k, {-1, -1, -1}, {0, 0, 0}, {0, 0, 0}, k, {1.0, 1.0, 1.0}};
      bool any = false;
      for (int kd = 0; kd < 3; kd++) {
        const auto& A = a.rows[kd];
        for (size_t r = 0; r < A.size(); r++)
          if (A[r].phase == i && A[r].k == k) {
            nd.row[kd] = (int32_t)r; nd.nk[kd] = A[r].nk; nd.row0[kd] = A[r].row0; nd.limit[kd] = A[r].limit;
            any = true;
          }
      }
      if (any) a.nodes.push_back(nd);
    }
  // ---- the per-vector record of gel_eval_batch_aero_device: two parts, each in gel_eval_aero_all's layout for ITS rows.
  //      Part A: nodes 1 .. n of the aerodynamic phases' "all nodes" specs -- what the fused kernel's lanes can write, a spec's row of
  //      a column n doubles long.  Part B: every other row.  Every section starts on a multiple of eight doubles.
  auto fusable = [&](const gel::AeroRowDev& r) { return p->ph[r.phase].air && r.nk == p->ph[r.phase].n + 1 && r.k >= 1; };
  for (int kd = 0; kd < 3; kd++) {
    const auto& A = a.rows[kd];
    a.part_of[kd].assign(A.size(), 0);
    for (size_t r0 = 0; r0 < A.size(); r0 += A[r0].nk) {
      // the spec's rows of part A and of part B, each a spec of its own there
      int rowA0 = (int)a.part_rows[0][kd].size(), rowB0 = (int)a.part_rows[1][kd].size(), nA = 0, nB = 0;
      for (int k = 0; k < A[r0].nk; k++) (fusable(A[r0 + k]) ? nA : nB)++;
      int iA = 0, iB = 0;
      for (int k = 0; k < A[r0].nk; k++) {
        const bool fa = fusable(A[r0 + k]);
        gel::AeroRowDev q = A[r0 + k];
        q.nk = fa ? nA : nB; q.row0 = fa ? rowA0 : rowB0;
        a.part_of[kd][r0 + k] = (fa ? 0 : 1) | ((fa ? rowA0 + iA : rowB0 + iB) << 1);   // part, row inside the part
        a.part_rows[fa ? 0 : 1][kd].push_back(q);
        (fa ? iA : iB)++;
      }
    }
  }
  int64_t off = 0;
  auto pad8 = [](int64_t v) { return (v + 7) / 8 * 8; };
  // part A, spec-major (gel_device.h AeroPhaseDev): one block of 13 n doubles per (kind, phase) spec
  for (int kd = 0; kd < 3; kd++) {
    const auto& A = a.part_rows[0][kd];
    a.partA_base[kd].assign(A.size(), 0);
    for (size_t r0 = 0; r0 < A.size(); r0 += A[r0].nk) {
      for (int k = 0; k < A[r0].nk; k++) a.partA_base[kd][r0 + k] = off;
      off = pad8(off + (int64_t)(p->fd_recompute ? gel::kAeroSpecColsWithT : gel::kAeroSpecCols) * A[r0].nk);
    }
  }
  {   // the dump area: where the lanes' stores of a kind their phase does not have go (AeroPhaseDev::base)
    int nmax = 0;
    for (const auto& h : p->ph) nmax = std::max(nmax, h.n);
    a.dump = off;
    off = pad8(off + (int64_t)gel::kAeroSpecColsWithT * nmax);
  }
  a.partA_len = off;
  // part B: gel_eval_aero_all's layout for its rows
  for (int kd = 0; kd < 3; kd++) { a.off_con[1][kd] = off; off = pad8(off + (int64_t)a.part_rows[1][kd].size()); }
  for (int kd = 0; kd < 3; kd++) { a.off_jac[1][kd] = off; off = pad8(off + (int64_t)a.part_rows[1][kd].size() * ((kd == 1) ? 8 : 12)); }
  for (int kd = 0; kd < 3; kd++) { a.off_con[0][kd] = 0; a.off_jac[0][kd] = 0; }
  a.ld = off;
  // node tables of the two parts.  Part A: row0 = first double of the spec's block in the record, row = the constraint value's place
  // (block + node), ko = the node's place in a column's row; part B: the ordinary tables of its own rows
  for (int part = 0; part < 2; part++) {
    auto& nodes_p = a.part_nodes[part];
    for (const auto& nd0 : a.nodes) {
      gel::AeroNodeDev nd = nd0;
      bool any = false;
      for (int kd = 0; kd < 3; kd++) {
        nd.row[kd] = -1;
        if (nd0.row[kd] < 0) continue;
        const int32_t po = a.part_of[kd][nd0.row[kd]];
        if ((po & 1) != part) continue;
        const auto& q = a.part_rows[part][kd][po >> 1];
        nd.ko = (po >> 1) - q.row0;
        nd.nk[kd] = q.nk;
        if (part == 0) {
          nd.row0[kd] = (int32_t)a.partA_base[kd][po >> 1];
          nd.row[kd] = nd.row0[kd] + nd.ko;
        } else {
          nd.row[kd] = po >> 1; nd.row0[kd] = q.row0;
        }
        any = true;
      }
      if (any) nodes_p.push_back(nd);
    }
  }
  // per-phase records of part A for the fused kernel's lanes
  a.ph.assign(p->ph.size(), gel::AeroPhaseDev{});
  for (size_t i = 0; i < p->ph.size(); i++) {
    gel::AeroPhaseDev& q = a.ph[i];
    for (int kd = 0; kd < 3; kd++) { q.il[kd] = 0.0; q.ilx[kd] = 0.0; q.base[kd] = (int32_t)(8 * a.dump); }
    for (int kd = 0; kd < 3; kd++) {
      const auto& A = a.part_rows[0][kd];
      for (size_t r0 = 0; r0 < A.size(); r0 += A[r0].nk) {
        if (A[r0].phase != (int)i) continue;
        q.kinds |= 1 << kd;
        q.base[kd] = (int32_t)(8 * a.partA_base[kd][r0]);
        q.il[kd] = 1.0 / A[r0].limit;            // the kernels' frcp(limit): the correctly rounded quotient
        q.ilx[kd] = q.il[kd] * p->dev.inv_dx;
      }
    }
  }
  if (8 * a.ld >= (int64_t)1 << 31) return fail(GEL_ERR_ARG, "aero record too long for 32-bit byte offsets");
  if (p->device != GEL_DEVICE_NONE) {
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(a.d_nodes.upload(a.nodes)); HIPCHK(a.d_ph.upload(a.ph));
    for (int part = 0; part < 2; part++)
      if (!a.part_nodes[part].empty()) HIPCHK(a.d_part_nodes[part].upload(a.part_nodes[part]));
  }
  gel_problem::Conprod cp;   // the K products' tables follow the new configuration (and stay the old ones if this fails)
  if (const int rc = conprod_build(p, p->lin_rows, p->fn_rows, a, cp)) return rc;
  if (p->device != GEL_DEVICE_NONE) HIPCHK(drain(p));   // launches in flight, on the handle's stream or on the caller's, still read the old tables
  p->aero = std::move(a);
  p->conprod = std::move(cp);
  return GEL_OK;
}

int gel_aero_record_layout(const gel_problem* p, int64_t* width, int64_t* off_con, int64_t* off_jac) {
  if (!p || !width || !off_con || !off_jac) return fail(GEL_ERR_ARG, "bad argument");
  *width = p->aero.ld;
  for (int part = 0; part < 2; part++)
    for (int k = 0; k < 3; k++) { off_con[3 * part + k] = p->aero.off_con[part][k]; off_jac[3 * part + k] = p->aero.off_jac[part][k]; }
  return GEL_OK;
}

// record index of every entry of gel_eval_aero_all's arrays: var = -1 the constraint vector [nrows], var 0..3 the position /
// velocity / quaternion / t block of the gradient values (in the order of gel_aero_pattern)
int gel_aero_record_map(const gel_problem* p, int32_t kind, int32_t var, int64_t* idx) {
  if (!p || kind < 0 || kind > 2 || var < -1 || var > 3 || !idx) return fail(GEL_ERR_ARG, "bad argument");
  aero_record_map_of(p, p->aero, kind, var, idx);
  return GEL_OK;
}

// Defect groups AND aero path constraints of a resident batch: d_res [B][11N], d_jvar [B][V] as gel_eval_batch_device writes them,
// d_aero [B][width] one record per vector (gel_aero_record_layout / gel_aero_record_map).
int gel_eval_batch_aero_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, double* d_aero,
                               void* stream) {
  if (!p || !d_x || B < 1 || !d_res || !d_jvar || !d_aero) return fail(GEL_ERR_ARG, "bad argument");
  if (p->exact && !p->exact_aero)   // the exact defect Jacobian has no fused form with the FORWARD-DIFFERENCE aero rows
    return fail(GEL_ERR_ARG, "gel_eval_batch_aero_device has no exact-Jacobian form (handle created with GEL_FLAG_EXACT_DEFECT_JAC)");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (p->aero.nodes.empty()) return fail(GEL_ERR_ARG, "no aero path constraints configured (gel_aero_configure)");
  hipStream_t s = stream_of(p, stream);
  gel::AeroLaunchOut out[2];
  for (int part = 0; part < 2; part++)
    for (int k = 0; k < 3; k++) {   // part A (spec-major): every pointer is the record itself
      out[part].nrows[k] = (int32_t)p->aero.part_rows[part][k].size();
      out[part].con[k] = out[part].nrows[k] ? d_aero + p->aero.off_con[part][k] : nullptr;
      out[part].jac[k] = out[part].nrows[k] ? d_aero + p->aero.off_jac[part][k] : nullptr;
    }
  // GEL_AERO_FUSED=0: the two kernels one after the other (same record, same bits)
  // GEL_FLAG_EXACT_AERO_JAC: the defect groups as gel_eval_batch_device forms them (launch_defects), then both parts of the record by
  // the values-only aero launches and the exact aero kernel; the fused AERO instantiation is not used
  const bool fused = !p->exact_aero && p->aero_fused && gel::eval_aero_fusable(p->dev, B) && !p->aero.part_nodes[0].empty();
  if (p->exact_aero) {
    HIPCHK(launch_defects(p, p->dev, B, d_x, d_res, d_jvar, s));
    HIPCHK(launch_aero_kinds(p, p->dev, (int)p->aero.part_nodes[0].size(), p->aero.d_part_nodes[0].get(), B, d_x, out[0], s, p->aero.ld, true));
  } else if (fused) {
    gel::ProblemDev dv = p->dev;
    dv.aero_ph = p->aero.d_ph.get(); dv.aero_out = d_aero; dv.aero_ld = p->aero.ld;
    HIPCHK(gel::launch_eval_aero(dv, B, d_x, d_res, d_jvar, s));
  } else {
    HIPCHK(gel::launch_eval(p->dev, B, d_x, d_res, d_jvar, s));
    HIPCHK(gel::launch_aero(p->dev, (int)p->aero.part_nodes[0].size(), p->aero.d_part_nodes[0].get(), B, d_x, out[0], s, p->aero.ld, true));
  }
  HIPCHK(launch_aero_kinds(p, p->dev, (int)p->aero.part_nodes[1].size(), p->aero.d_part_nodes[1].get(), B, d_x, out[1], s, p->aero.ld, false, true));
  return GEL_OK;
}

// which form aero_kernel's launcher takes for B vectors (gel::aero_form, the function launch_aero itself decides by); no stream, no
// device: host-only handles answer too
int gel_aero_launch_info(const gel_problem* p, int32_t B, int32_t records, int64_t* info) {
  if (!p || !info || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  int32_t nrows[3];
  for (int k = 0; k < 3; k++) nrows[k] = (int32_t)(records ? p->aero.part_rows[0][k].size() : p->aero.rows[k].size());
  const int nnodes = (int)(records ? p->aero.part_nodes[0].size() : p->aero.nodes.size());
  const gel::AeroForm f = gel::aero_form(nnodes, B, nrows, records ? p->aero.ld : 0);
  info[0] = f.flat; info[1] = f.runs; info[2] = f.run_len; info[3] = f.max_bytes;
  return GEL_OK;
}

int gel_aero_dims(const gel_problem* p, int32_t kind, int32_t* nrows, int64_t* nnz4) {
  if (!p || kind < 0 || kind > 2 || !nrows || !nnz4) return fail(GEL_ERR_ARG, "bad argument");
  const int64_t R = (int64_t)p->aero.rows[kind].size();
  *nrows = (int32_t)R;
  nnz4[0] = 3 * R; nnz4[1] = 3 * R; nnz4[2] = (kind == 1) ? 0 : 4 * R; nnz4[3] = 2 * R;
  return GEL_OK;
}

int gel_aero_pattern(const gel_problem* p, int32_t kind, int32_t var, int32_t* rows, int32_t* cols) {
  if (!p || kind < 0 || kind > 2 || var < 0 || var > 3 || !rows || !cols) return fail(GEL_ERR_ARG, "bad argument");
  aero_pattern_of(p, p->aero, kind, var, rows, cols);
  return GEL_OK;
}

int gel_eval_aero_all_device(gel_problem* p, int32_t B, const double* d_x, double* const* d_con, double* const* d_jac,
                             void* stream) {
  if (!p || B < 1 || !d_x || !d_con) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  gel::AeroLaunchOut out;
  for (int k = 0; k < 3; k++) {
    out.nrows[k] = (int32_t)p->aero.rows[k].size();
    out.con[k] = out.nrows[k] ? d_con[k] : nullptr;
    out.jac[k] = (out.con[k] && d_jac) ? d_jac[k] : nullptr;
  }
  HIPCHK(launch_aero_kinds(p, p->dev, (int)p->aero.nodes.size(), p->aero.d_nodes.get(), B, d_x, out, stream_of(p, stream)));
  return GEL_OK;
}

int gel_eval_aero_all(gel_problem* p, int32_t B, const double* x, double* const* con, double* const* jac) {
  if (!p || B < 1 || !x || !con) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (p->aero.nodes.empty()) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  // x and one output area: con[0] | jac[0] | con[1] | jac[1] | con[2] | jac[2] (only what was asked for; small calls are the
  // optimiser's callback)
  gel::AeroLaunchOut out;
  StagedBuf oc[3], oj[3];
  for (int k = 0; k < 3; k++) {
    const size_t R = p->aero.rows[k].size();
    out.nrows[k] = (int32_t)R;
    oc[k] = staged_out(R ? con[k] : nullptr, (size_t)B * R);
    oj[k] = staged_out((oc[k].dst && jac) ? jac[k] : nullptr, (size_t)B * aero_jac_len(p, k));
  }
  if (!oc[0].dst && !oc[1].dst && !oc[2].dst) return GEL_OK;
  return staged_call(p, kStagedZeroCopy, {staged_in(x, (size_t)B * p->dims.num_vars), oc[0], oj[0], oc[1], oj[1], oc[2], oj[2]},
                     [&](const gel::ProblemDev& dv, double* const* a) -> int {
                       for (int k = 0; k < 3; k++) { out.con[k] = a[1 + 2 * k]; out.jac[k] = a[2 + 2 * k]; }
                       HIPCHK(launch_aero_kinds(p, dv, (int)p->aero.nodes.size(), p->aero.d_nodes.get(), B, a[0], out, p->stream.get()));
                       return GEL_OK;
                     });
}

int gel_eval_aero(gel_problem* p, int32_t kind, int32_t B, const double* x, double* con, double* jac_vals) {
  if (!p || kind < 0 || kind > 2 || B < 1 || !x || !con) return fail(GEL_ERR_ARG, "bad argument");
  double* c[3] = {nullptr, nullptr, nullptr};
  double* j[3] = {nullptr, nullptr, nullptr};
  c[kind] = con; j[kind] = jac_vals;
  return gel_eval_aero_all(p, B, x, c, j);
}

// ------------- knot / terminal / user rows (lib/con_init_terminal_knot.py, example/user_constraints.py) -------------
int gel_rows_configure(gel_problem* p, int32_t nlin, const gel_linear_row* lin, int32_t nfn, const gel_nodefn_row* fn) {
  if (!p || nlin < 0 || nfn < 0 || (nlin && !lin) || (nfn && !fn)) return fail(GEL_ERR_ARG, "bad argument");
  for (int i = 0; i < nlin; i++)
    if (lin[i].idx0 < 0 || lin[i].idx0 >= p->dims.num_vars || lin[i].idx1 >= p->dims.num_vars)
      return fail(GEL_ERR_ARG, "linear row: variable index out of range");
  for (int i = 0; i < nfn; i++)
    if (fn[i].fn < 0 || fn[i].fn > 15 || fn[i].node < 0 || fn[i].node >= p->dims.M || !(fn[i].p[0] != 0.0) ||
        fn[i].tcol < -1 || fn[i].tcol > p->dims.S || (fn[i].fn >= 9 && fn[i].tcol < 0) || (fn[i].mode & ~15) || (fn[i].mode & 3) > 1)
      return fail(GEL_ERR_ARG, "node-function row: unknown function or mode, node / time column out of range, or zero scale");
  // the new tables in locals, swapped in only once everything has succeeded: a failed call leaves the old ones in place
  std::vector<gel::LinRowDev> lin_rows(nlin);
  std::vector<gel::FnRowDev> fn_rows(nfn);
  for (int i = 0; i < nlin; i++) lin_rows[i] = gel::LinRowDev{lin[i].idx0, lin[i].idx1 < 0 ? -1 : lin[i].idx1, lin[i].coef0, lin[i].coef1, lin[i].c0};
  for (int i = 0; i < nfn; i++) {
    gel::FnRowDev& d = fn_rows[i];
    d.fn = fn[i].fn; d.node = fn[i].node; d.tcol = fn[i].tcol; d.mode = fn[i].mode;
    for (int k = 0; k < 8; k++) d.p[k] = fn[i].p[k];
  }
  DeviceArray<gel::LinRowDev> d_lin;
  DeviceArray<gel::FnRowDev> d_fn;
  if (p->device != GEL_DEVICE_NONE) {
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(d_lin.upload(lin_rows)); HIPCHK(d_fn.upload(fn_rows));
  }
  gel_problem::Conprod cp;   // the K products' tables follow the new rows (and stay the old ones if this fails)
  if (const int rc = conprod_build(p, lin_rows, fn_rows, p->aero, cp)) return rc;
  if (p->device != GEL_DEVICE_NONE) HIPCHK(drain(p));   // launches in flight, on the handle's stream or on the caller's, still read the old tables
  p->lin_rows = std::move(lin_rows); p->fn_rows = std::move(fn_rows);
  p->d_lin_rows = std::move(d_lin); p->d_fn_rows = std::move(d_fn);
  p->conprod = std::move(cp);
  return GEL_OK;
}

int gel_rows_dims(const gel_problem* p, int32_t* nlin, int32_t* nfn) {
  if (!p || !nlin || !nfn) return fail(GEL_ERR_ARG, "null argument");
  *nlin = (int32_t)p->lin_rows.size();
  *nfn = (int32_t)p->fn_rows.size();
  return GEL_OK;
}

int gel_rows_eval_device(gel_problem* p, int32_t B, const double* d_x, double* d_con, double* d_jfn, void* stream) {
  if (!p || B < 1 || !d_x || !d_con) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(launch_rows_kinds(p, p->dev, B, d_x, d_con, d_jfn, stream_of(p, stream)));
  return GEL_OK;
}


int gel_rows_eval(gel_problem* p, int32_t B, const double* x, double* con, double* jfn) {
  if (!p || B < 1 || !x || !con) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  const size_t R = p->lin_rows.size() + p->fn_rows.size(), nf = p->fn_rows.size();
  if (R == 0) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  // small calls are the optimiser's callback
  return staged_call(p, kStagedZeroCopy, {staged_in(x, (size_t)B * p->dims.num_vars), staged_out(con, (size_t)B * R), staged_out(jfn, (size_t)B * nf * 7)},
                     [&](const gel::ProblemDev& dv, double* const* a) -> int {
                       HIPCHK(launch_rows_kinds(p, dv, B, a[0], a[1], a[2], p->stream.get()));
                       return GEL_OK;
                     });
}

// ------------- products with K, the Jacobian of every row that is not a defect row -------------
int gel_con_products_dims(const gel_problem* p, int64_t* info) {
  if (!p || !info) return fail(GEL_ERR_ARG, "null argument");
  const gel_problem::Conprod& c = p->conprod;
  info[0] = c.R; info[1] = c.nlin; info[2] = c.nfn;
  for (int k = 0; k < 3; k++) info[3 + k] = c.nrows[k];
  info[6] = c.nnz; info[7] = c.max_row; info[8] = c.max_col;
  return GEL_OK;
}

// the argument rules every form shares
static int conprod_check(const gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                         const void* in, const void* out) {
  if (!p || B < 1 || !in || !out) return fail(GEL_ERR_ARG, "bad argument");
  const gel_problem::Conprod& c = p->conprod;
  if (c.R == 0) return fail(GEL_ERR_ARG, "K products: no rows configured (gel_rows_configure, gel_aero_configure)");
  if (c.nfn && !jfn) return fail(GEL_ERR_ARG, "K products: jfn is required when the row table has node-function rows");
  const bool any_aero = c.nrows[0] || c.nrows[1] || c.nrows[2];
  if (!any_aero) {
    if (aero_jac || aero_record) return fail(GEL_ERR_ARG, "K products: no aero kind has rows, aero_jac and aero_record must be NULL");
    return GEL_OK;
  }
  if ((aero_jac != nullptr) == (aero_record != nullptr))
    return fail(GEL_ERR_ARG, "K products: exactly one of aero_jac and aero_record must be given");
  if (aero_jac)
    for (int k = 0; k < 3; k++)
      if (c.nrows[k] && !aero_jac[k]) return fail(GEL_ERR_ARG, "K products: aero_jac of a kind with rows is NULL");
  return GEL_OK;
}

static gel::ConprodVals conprod_vals(const gel_problem* p, const double* jfn, const double* const* aero_jac, const double* aero_record) {
  const gel_problem::Conprod& c = p->conprod;
  gel::ConprodVals v{};
  v.jfn = c.nfn ? jfn : nullptr;
  v.jfn_stride = c.nfn ? (int64_t)c.nfn * 7 : 0;
  for (int k = 0; k < 3; k++) {
    const bool has = c.nrows[k] != 0;
    v.aero[k] = !has ? nullptr : (aero_record ? aero_record : aero_jac[k]);
    v.aero_stride[k] = !has ? 0 : (aero_record ? p->aero.ld : c.jac_len[k]);
  }
  return v;
}

int gel_con_products_host(const gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                          const double* in, double* out, int32_t transpose, int32_t accumulate) {
  if (const int rc = conprod_check(p, B, jfn, aero_jac, aero_record, in, out)) return rc;
  const gel_problem::Conprod& c = p->conprod;
  const gel_problem::Conprod::Dir& D = c.dir[transpose ? 1 : 0];
  const gel::ConprodVals v = conprod_vals(p, jfn, aero_jac, aero_record);
  const std::vector<int64_t>& off = aero_record ? D.offr : D.offd;
  const size_t nin = transpose ? (size_t)c.R : (size_t)p->dims.num_vars, nout = transpose ? (size_t)p->dims.num_vars : (size_t)c.R;
  int rc = GEL_OK;
  for (int32_t b = 0; b < B; b++) {
    const double* ib = in + (size_t)b * nin;
    double* ob = out + (size_t)b * nout;
    for (size_t o = 0; o < nout; o++) {   // the same chain as a lane of conprod_kernel
      double acc = 0.0;
      for (int32_t e = D.ptr[o]; e < D.ptr[o + 1]; e++) {
        const int sc = D.src[e];
        const double a = (sc == gel::kConSrcConst) ? D.cval[e]
                       : (sc == gel::kConSrcJfn)   ? v.jfn[(size_t)b * v.jfn_stride + off[e]]
                                                   : v.aero[sc - gel::kConSrcAero0][(size_t)b * v.aero_stride[sc - gel::kConSrcAero0] + off[e]];
        acc = std::fma(a, ib[D.idx[e]], acc);
      }
      if (accumulate) acc = ob[o] + acc;
      ob[o] = acc;
      if (!std::isfinite(acc)) rc = GEL_NONFINITE;
    }
  }
  return rc;
}

static int conprod_device(gel_problem* p, int32_t B, const double* d_jfn, const double* const* d_aero_jac, const double* d_aero_record,
                          const double* d_in, double* d_out, int transpose, int accumulate, hipStream_t s) {
  const gel_problem::Conprod& c = p->conprod;
  const gel_problem::Conprod::Dir& D = c.dir[transpose ? 1 : 0];
  gel::ConprodOpDev op{};
  op.nout = transpose ? p->dims.num_vars : (int32_t)c.R;
  op.nin = transpose ? (int32_t)c.R : p->dims.num_vars;
  op.ptr = D.d_ptr.get(); op.idx = D.d_idx.get(); op.src = D.d_src.get(); op.cval = D.d_cval.get();
  op.off = d_aero_record ? D.d_offr.get() : D.d_offd.get();
  HIPCHK(gel::launch_conprod(op, conprod_vals(p, d_jfn, d_aero_jac, d_aero_record), B, d_in, d_out, accumulate, p->d_flag.get(), s));
  return GEL_OK;
}

int gel_con_matvec_device(gel_problem* p, int32_t B, const double* d_jfn, const double* const* d_aero_jac, const double* d_aero_record,
                          const double* d_v, double* d_y) {
  if (const int rc = conprod_check(p, B, d_jfn, d_aero_jac, d_aero_record, d_v, d_y)) return rc;
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuConprod);
  HIPCHK(hipSetDevice(p->device));
  return conprod_device(p, B, d_jfn, d_aero_jac, d_aero_record, d_v, d_y, 0, 0, p->stream.get());
}

int gel_con_rmatvec_device(gel_problem* p, int32_t B, const double* d_jfn, const double* const* d_aero_jac, const double* d_aero_record,
                           const double* d_lam, double* d_g, int32_t accumulate) {
  if (const int rc = conprod_check(p, B, d_jfn, d_aero_jac, d_aero_record, d_lam, d_g)) return rc;
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuConprod);
  HIPCHK(hipSetDevice(p->device));
  return conprod_device(p, B, d_jfn, d_aero_jac, d_aero_record, d_lam, d_g, 1, accumulate != 0, p->stream.get());
}

// host buffers: copy in, one launch, copy out, one synchronise
static int conprod_hostbuf(gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                           const double* in, double* out, int transpose, int accumulate) {
  if (const int rc = conprod_check(p, B, jfn, aero_jac, aero_record, in, out)) return rc;
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuConprod);
  HIPCHK(hipSetDevice(p->device));
  const gel_problem::Conprod& c = p->conprod;
  const size_t ni = (size_t)B * (transpose ? (size_t)c.R : (size_t)p->dims.num_vars), no = (size_t)B * (transpose ? (size_t)p->dims.num_vars : (size_t)c.R);
  // the values: jfn when there are node-function rows; the record, or the dense array of every kind that has rows
  StagedBuf aero[3];
  for (int k = 0; k < 3; k++)
    aero[k] = (aero_record && k == 0) ? staged_in(aero_record, (size_t)B * (size_t)p->aero.ld)
                                      : staged_in((aero_jac && c.nrows[k]) ? aero_jac[k] : nullptr, (size_t)B * (size_t)c.jac_len[k]);
  return staged_call(p, 0, {staged_in(in, ni), accumulate ? staged_inout(out, no) : staged_out(out, no),
                            staged_in(c.nfn ? jfn : nullptr, (size_t)B * c.nfn * 7), aero[0], aero[1], aero[2]},
                     [&](const gel::ProblemDev&, double* const* a) {
                       return conprod_device(p, B, a[2], aero_jac ? a + 3 : nullptr, aero_record ? a[3] : nullptr, a[0], a[1], transpose,
                                             accumulate, p->stream.get());
                     });
}

int gel_con_matvec(gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record, const double* v,
                   double* y) {
  return conprod_hostbuf(p, B, jfn, aero_jac, aero_record, v, y, 0, 0);
}
int gel_con_rmatvec(gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                    const double* lam, double* g, int32_t accumulate) {
  return conprod_hostbuf(p, B, jfn, aero_jac, aero_record, lam, g, 1, accumulate != 0);
}

}  // extern "C"
