// gel_host_jprod.hip -- the Jacobian products from the compact values (gel_jac_products_*, gel_jac_[r]matvec*):
// the operator tables, built from the pattern walk at gel_problem_create, the host product and the device forms.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <vector>

#include "gel_host_handle.h"

using namespace gelhost;

namespace gelhost {

// ---- operator tables of the Jacobian products (gel_jprod.h) ----
// Built from walk_pattern() and nothing else: every COO entry goes, with its global row and column, to the phase that owns its
// row; explicit zeros of the pattern are dropped.  Returns a message on a pattern the decomposition does not cover (a column but
// a time column shared by two phases), else null.
const char* build_jprod_tables(gel_problem& P) {
  static const int kBlockGroup[GEL_NUM_BLOCKS] = {0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3};
  static const int kBlockVar[GEL_NUM_BLOCKS] = {0, 5, 1, 2, 5, 0, 1, 2, 3, 5, 3, 4, 5};   // mass, position, velocity, quaternion, u, t
  static const int kRowMult[4] = {1, 3, 3, 4};
  const int S = (int)P.ph.size(), N = P.dims.N, M = P.dims.M, nvars = P.dims.num_vars;
  const int64_t row_off[4] = {0, N, 4 * (int64_t)N, 7 * (int64_t)N};
  const int64_t var_off[6] = {0, M, 4 * (int64_t)M, 7 * (int64_t)M, 11 * (int64_t)M, 11 * (int64_t)M + 2 * (int64_t)N};
  const int tcol0 = (int)var_off[5];
  std::vector<int32_t> node_phase((size_t)N);
  for (int i = 0; i < S; i++)
    for (int j = 0; j < P.ph[i].n; j++) node_phase[(size_t)P.ph[i].ua + j] = i;
  // local numbering: rows [mass n | pos 3n | vel 3n | quat 4n] of the phase, columns as phase_columns() (to, tf last)
  std::vector<int32_t> row_local((size_t)11 * N, -1), col_local((size_t)nvars, -1), col_phase((size_t)nvars, -1);
  std::vector<std::vector<int32_t>> rowmap((size_t)S), colmap((size_t)S);
  for (int i = 0; i < S; i++) {
    const HostPhase& h = P.ph[i];
    for (int g = 0; g < 4; g++)
      for (int k = 0; k < kRowMult[g] * h.n; k++) {
        const int32_t r = (int32_t)(row_off[g] + (int64_t)kRowMult[g] * h.ua + k);
        row_local[(size_t)r] = (int32_t)rowmap[i].size();
        rowmap[i].push_back(r);
      }
    phase_columns(&P, i, colmap[i]);
    for (size_t l = 0; l + 2 < colmap[i].size(); l++) {
      const int32_t c = colmap[i][l];
      if (c < 0 || c >= tcol0 || col_local[(size_t)c] >= 0) return "internal: a state or control column belongs to two phases";
      col_local[(size_t)c] = (int32_t)l;
      col_phase[(size_t)c] = i;
    }
  }
  struct Ent { int32_t in; int32_t slot; double cv; };   // slot < 0: constant cv; else 2 * (slot - voff) + negated
  std::vector<std::vector<std::vector<Ent>>> fw((size_t)S), bw((size_t)S);
  std::vector<std::vector<Ent>> tc((size_t)2 * S);
  for (int i = 0; i < S; i++) { fw[i].resize(rowmap[i].size()); bw[i].resize(colmap[i].size() - 2); }
  std::vector<int64_t> rlen((size_t)11 * N, 0), clen((size_t)nvars, 0);
  const char* err = nullptr;
  int64_t nconst = 0, nvarent = 0;
  walk_pattern(P, [&](int blk, int64_t, int32_t r, int32_t c, int kind, double cv, int64_t slot) {
    if (kind == 0 && cv == 0.0) return;   // an explicit zero of the reference's pattern
    const int g = kBlockGroup[blk];
    const int64_t gr = row_off[g] + r, gc = var_off[kBlockVar[blk]] + c;
    const int i = node_phase[(size_t)(r / kRowMult[g])];
    const HostPhase& h = P.ph[i];
    const int32_t lr = row_local[(size_t)gr];
    int32_t lc, side = -1;
    if (gc >= tcol0) {
      side = (int32_t)(gc - tcol0) - i;
      if (side != 0 && side != 1) { err = "internal: a time column outside its phase"; return; }
      lc = (int32_t)colmap[i].size() - 2 + side;
    } else {
      if (col_phase[(size_t)gc] != i) { err = "internal: an entry couples two phases"; return; }
      lc = col_local[(size_t)gc];
    }
    int32_t sl = -1;
    if (kind != 0) {
      const int64_t off = slot - h.voff;
      if (off < 0 || off > (int64_t)h.K * h.n) { err = "internal: a compact slot outside its phase"; return; }
      sl = (int32_t)(2 * off + (kind == 2 ? 1 : 0));
      nvarent++;
    } else
      nconst++;
    fw[i][(size_t)lr].push_back({lc, sl, cv});
    if (side >= 0) tc[(size_t)2 * i + side].push_back({lr, sl, cv});
    else bw[i][(size_t)lc].push_back({lr, sl, cv});
    rlen[(size_t)gr]++; clen[(size_t)gc]++;
  });
  if (err) return err;
  P.jp.info[0] = nconst; P.jp.info[1] = nvarent;
  P.jp.info[2] = *std::max_element(rlen.begin(), rlen.end());
  P.jp.info[3] = *std::max_element(clen.begin(), clen.end());

  std::vector<int32_t>& it = P.jp.it;
  std::vector<double>& dt = P.jp.dt;
  it.clear(); dt.clear();
  P.jp.ph.assign((size_t)S, gel::JprodPhaseDev{});
  P.jp.nin_max[0] = P.jp.nin_max[1] = 0;
  auto emit = [&](const std::vector<std::vector<Ent>>& rows, const std::vector<int32_t>& omap, const std::vector<int32_t>& imap,
                  size_t nin, gel::JprodOpDev& op) {
    const size_t nout = rows.size();
    std::vector<int32_t> ncs(nout, 0), nvs(nout, 0);
    size_t cw = 0, vw = 0;
    for (size_t o = 0; o < nout; o++) {
      for (const Ent& e : rows[o]) (e.slot < 0 ? ncs[o] : nvs[o])++;
      cw = std::max(cw, (size_t)ncs[o]); vw = std::max(vw, (size_t)nvs[o]);
    }
    // outputs with the same sequence of constant coefficients share one row of cval
    std::map<std::vector<double>, int32_t> seen;
    std::vector<int32_t> vrow(nout, 0);
    std::vector<double> key;
    for (size_t o = 0; o < nout; o++) {
      key.clear();
      for (const Ent& e : rows[o]) if (e.slot < 0) key.push_back(e.cv);
      vrow[o] = seen.emplace(key, (int32_t)seen.size()).first->second;
    }
    const size_t nvr = seen.size();
    op.nout = (int32_t)nout; op.nin = (int32_t)nin; op.cw = (int32_t)cw; op.vw = (int32_t)vw; op.nvr = (int32_t)nvr; op.pad = 0;
    op.cnt = (int64_t)it.size();
    it.insert(it.end(), ncs.begin(), ncs.end()); it.insert(it.end(), nvs.begin(), nvs.end());
    const size_t cw4 = (cw + 3) & ~(size_t)3;
    while (it.size() & 3) it.push_back(0);   // 16-byte alignment of the packed indices
    op.cidx = (int64_t)it.size(); it.resize(it.size() + cw4 * nout, 0);
    op.vidx = (int64_t)it.size(); it.resize(it.size() + vw * nout, 0);
    op.vslot = (int64_t)it.size(); it.resize(it.size() + vw * nout, 0);
    op.omap = (int64_t)it.size(); it.insert(it.end(), omap.begin(), omap.begin() + nout);
    op.imap = (int64_t)it.size(); it.insert(it.end(), imap.begin(), imap.begin() + nin);
    op.vrow = (int64_t)it.size(); it.insert(it.end(), vrow.begin(), vrow.end());
    if (dt.size() & 1) dt.push_back(0.0);
    op.cval = (int64_t)dt.size(); dt.resize(dt.size() + cw4 * nvr, 0.0);
    for (size_t o = 0; o < nout; o++) {
      size_t ec = 0, ev = 0;
      for (const Ent& e : rows[o]) {
        if (e.slot < 0) {
          it[(size_t)op.cidx + gel::jprod_cidx_at((int)ec, (int)nout, (int)o)] = e.in;
          dt[(size_t)op.cval + gel::jprod_cval_at((int)ec, (int)nvr, vrow[o])] = e.cv;
          ec++;
        }
        else { it[(size_t)op.vidx + ev * nout + o] = e.in; it[(size_t)op.vslot + ev * nout + o] = e.slot; ev++; }
      }
    }
  };
  for (int i = 0; i < S; i++) {
    gel::JprodPhaseDev& q = P.jp.ph[i];
    q.voff = P.ph[i].voff;
    emit(fw[i], rowmap[i], colmap[i], colmap[i].size(), q.fw);
    emit(bw[i], colmap[i], rowmap[i], rowmap[i].size(), q.bw);
    for (int side = 0; side < 2; side++) {
      const std::vector<Ent>& t = tc[(size_t)2 * i + side];
      gel::JprodTcolDev& d = q.tc[side];
      d.nt = (int32_t)t.size(); d.pad = 0;
      d.ridx = (int64_t)it.size(); for (const Ent& e : t) it.push_back(e.in);
      d.tslot = (int64_t)it.size(); for (const Ent& e : t) it.push_back(e.slot);
      d.tval = (int64_t)dt.size(); for (const Ent& e : t) dt.push_back(e.slot < 0 ? e.cv : 0.0);
    }
    P.jp.nin_max[0] = std::max(P.jp.nin_max[0], q.fw.nin);
    P.jp.nin_max[1] = std::max(P.jp.nin_max[1], q.bw.nin);
  }
  gel::JprodDev& jd = P.jp.dev;
  jd.S = S; jd.V = (int32_t)P.dims.num_var_entries; jd.nvars = nvars; jd.nres = 11 * N; jd.tcol0 = tcol0; jd.pad = 0;
  jd.ph = nullptr; jd.it = nullptr; jd.dt = nullptr;
  return nullptr;
}

}  // namespace gelhost

namespace {

// One operator of one phase on the host, from the same tables and in the same order as a lane of jprod_kernel
void jprod_host_op(const gel_problem& P, const gel::JprodOpDev& op, int64_t voff, const double* jv, const double* in, double* out) {
  const int32_t* it = P.jp.it.data();
  const double* dt = P.jp.dt.data();
  const size_t nout = (size_t)op.nout;
  for (size_t o = 0; o < nout; o++) {
    double acc = 0.0;
    const int nc = it[(size_t)op.cnt + o], nv = it[(size_t)op.cnt + nout + o];
    for (int e = 0; e < nc; e++)
      acc = std::fma(dt[(size_t)op.cval + gel::jprod_cval_at(e, op.nvr, it[(size_t)op.vrow + o])],
                     in[it[(size_t)op.imap + it[(size_t)op.cidx + gel::jprod_cidx_at(e, op.nout, (int)o)]]], acc);
    for (int e = 0; e < nv; e++) {
      const int sl = it[(size_t)op.vslot + e * nout + o];
      const double a = jv[voff + (sl >> 1)];
      acc = std::fma((sl & 1) ? -a : a, in[it[(size_t)op.imap + it[(size_t)op.vidx + e * nout + o]]], acc);
    }
    out[it[(size_t)op.omap + o]] = acc;
  }
}
constexpr const char* kNoGpuJprod = "host-only handle: the device products need a GPU (gel_jac_products_host runs on the host)";

}  // namespace

extern "C" {

// ------------- Jacobian products from the compact values -------------
#define NEED_JPROD(p, t)                                                                                                  \
  do {                                                                                                                    \
    if (!gel::jprod_vectors_per_group((p)->jp.nin_max[(t) ? 1 : 0], (t) != 0))                                             \
      return fail(GEL_ERR_ARG, "Jacobian products: a phase's slice of the input does not fit a workgroup's LDS");          \
  } while (0)

int gel_jac_products_info(const gel_problem* p, int64_t* info) {
  if (!p || !info) return fail(GEL_ERR_ARG, "null argument");
  for (int k = 0; k < 4; k++) info[k] = p->jp.info[k];
  return GEL_OK;
}

int gel_jac_products_host(const gel_problem* p, int32_t B, const double* jvar, const double* in, double* out, int32_t transpose) {
  if (!p || B < 1 || !jvar || !in || !out) return fail(GEL_ERR_ARG, "bad argument");
  const size_t V = (size_t)p->dims.num_var_entries, nv = (size_t)p->dims.num_vars, nr = (size_t)11 * p->dims.N;
  const int S = p->dims.S;
  const int32_t* it = p->jp.it.data();
  const double* dt = p->jp.dt.data();
  int rc = GEL_OK;
  for (int32_t b = 0; b < B; b++) {
    const double* jv = jvar + (size_t)b * V;
    const double* ib = in + (size_t)b * (transpose ? nr : nv);
    double* ob = out + (size_t)b * (transpose ? nv : nr);
    for (int i = 0; i < S; i++) {
      const gel::JprodPhaseDev& q = p->jp.ph[i];
      jprod_host_op(*p, transpose ? q.bw : q.fw, q.voff, jv, ib, ob);
    }
    if (transpose) {
      // the time columns: the tf side of phase i - 1, then the to side of phase i, each summed in table order
      double* g = ob + p->jp.dev.tcol0;
      for (int i = 0; i <= S; i++) g[i] = 0.0;
      for (int i = 0; i < S; i++)
        for (int side = 0; side < 2; side++) {
          const gel::JprodPhaseDev& q = p->jp.ph[i];
          const gel::JprodTcolDev& t = q.tc[side];
          double acc = 0.0;
          for (int e = 0; e < t.nt; e++) {
            const int sl = it[(size_t)t.tslot + e];
            const double lam = ib[it[(size_t)q.bw.imap + it[(size_t)t.ridx + e]]];
            const double a = sl < 0 ? dt[(size_t)t.tval + e] : ((sl & 1) ? -jv[q.voff + (sl >> 1)] : jv[q.voff + (sl >> 1)]);
            acc = std::fma(a, lam, acc);
          }
          if (side == 0) g[i] = (i == 0) ? acc : g[i] + acc;
          else g[i + 1] = acc;
        }
    }
    const size_t no = transpose ? nv : nr;
    for (size_t k = 0; k < no; k++)
      if (!std::isfinite(ob[k])) { rc = GEL_NONFINITE; break; }
  }
  return rc;
}

// Vectors per workgroup of a product launch (what gel_jac_products_launch_info reports): the most whose staged inputs fit, or
// GEL_JPROD_VB = 1 / 2 / 4 / 8 (measurement switch, read per call; a value whose staged inputs do not fit is ignored).  The results
// do not depend on it.  0: not even one vector fits (NEED_JPROD).
static int jprod_vb(const gel_problem* p, int transpose) {
  const int nin = p->jp.nin_max[transpose ? 1 : 0];
  if (const char* e = getenv("GEL_JPROD_VB")) {
    const int w = atoi(e);
    if ((w == 1 || w == 2 || w == 4 || w == 8) && gel::jprod_lds_bytes(nin, w, transpose != 0) <= gel::kJprodMaxLds) return w;
  }
  return gel::jprod_vectors_per_group(nin, transpose != 0);
}

static int jprod_device(gel_problem* p, int32_t B, const double* d_jvar, const double* d_in, double* d_out, int transpose, hipStream_t s) {
  if (transpose) GROW_AFTER_DRAIN(p, p->jp.d_tpart, (size_t)B * p->dims.S * 2);   // an earlier product in flight still sums through the old workspace
  HIPCHK(gel::launch_jprod(p->jp.dev, p->jp.nin_max[transpose ? 1 : 0], B, d_jvar, d_in, d_out, p->jp.d_tpart.get(), p->d_flag.get(),
                           transpose, jprod_vb(p, transpose), p->jp.threads, s));
  return GEL_OK;
}

int gel_jac_products_launch_info(const gel_problem* p, int32_t* info) {
  if (!p || !info) return fail(GEL_ERR_ARG, "null argument");
  for (int t = 0; t < 2; t++) { info[2 * t] = jprod_vb(p, t); info[2 * t + 1] = p->jp.threads; }
  return GEL_OK;
}

int gel_jac_matvec_device(gel_problem* p, int32_t B, const double* d_jvar, const double* d_v, double* d_y, void* stream) {
  if (!p || B < 1 || !d_jvar || !d_v || !d_y) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuJprod);
  NEED_JPROD(p, 0);
  HIPCHK(hipSetDevice(p->device));
  return jprod_device(p, B, d_jvar, d_v, d_y, 0, stream_of(p, stream));
}

int gel_jac_rmatvec_device(gel_problem* p, int32_t B, const double* d_jvar, const double* d_lam, double* d_g, void* stream) {
  if (!p || B < 1 || !d_jvar || !d_lam || !d_g) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuJprod);
  NEED_JPROD(p, 1);
  HIPCHK(hipSetDevice(p->device));
  return jprod_device(p, B, d_jvar, d_lam, d_g, 1, stream_of(p, stream));
}

static int jprod_hostbuf(gel_problem* p, int32_t B, const double* jvar, const double* in, double* out, int transpose) {
  if (!p || B < 1 || !jvar || !in || !out) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuJprod);
  NEED_JPROD(p, transpose);
  HIPCHK(hipSetDevice(p->device));
  const size_t nv = (size_t)B * p->dims.num_vars, nr = (size_t)B * 11 * p->dims.N;
  return staged_call(p, 0, {staged_in(jvar, (size_t)B * p->dims.num_var_entries), staged_in(in, transpose ? nr : nv), staged_out(out, transpose ? nv : nr)},
                     [&](const gel::ProblemDev&, double* const* a) { return jprod_device(p, B, a[0], a[1], a[2], transpose, p->stream.get()); });
}

int gel_jac_matvec(gel_problem* p, int32_t B, const double* jvar, const double* v, double* y) { return jprod_hostbuf(p, B, jvar, v, y, 0); }
int gel_jac_rmatvec(gel_problem* p, int32_t B, const double* jvar, const double* lam, double* g) { return jprod_hostbuf(p, B, jvar, lam, g, 1); }

}  // extern "C"
