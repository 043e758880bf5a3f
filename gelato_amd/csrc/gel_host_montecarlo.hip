// gel_host_montecarlo.hip -- what is computed over the flights of a Monte-Carlo batch: the batched output table with envelope and
// peaks (gel_output_table_batch*; DESIGN.md 3.16, under a wind ensemble 3.19), the exact quantiles (gel_batch_quantiles*; 3.17)
// and the co-moments (gel_batch_comoments*; 3.18).
#include <algorithm>
#include <cstdlib>
#include <string>

#include "gel_outbatch.h"
#include "gel_quant.h"
#include "gel_comom.h"
#include "gel_host_handle.h"

using namespace gelhost;

extern "C" {

// ------------- batched post-processing table with envelope and peaks -------------
// the argument checks of both forms, before the device check; fills the column map
static int outbatch_check(gel_problem* p, int32_t B, const void* x, int32_t ncols, const int32_t* cols, const void* out, const void* env,
                          const void* peaks, gel::OutColsDev& C) {
  if (!p) return fail(GEL_ERR_ARG, "gel_output_table_batch: null handle");
  if (B < 0) return fail(GEL_ERR_ARG, "gel_output_table_batch: B < 0");
  if (B > 0 && !x) return fail(GEL_ERR_ARG, "gel_output_table_batch: x is NULL with B > 0");
  if (!out && !env && !peaks) return fail(GEL_ERR_ARG, "gel_output_table_batch: no output selected (out, env and peaks are all NULL)");
  bool seen[gel::kOutputColumns] = {};
  for (int c = 0; c < gel::kOutputColumns; c++) C.col[c] = (int8_t)c;
  C.ncols = gel::kOutputColumns;
  unsigned long long mask = ~0ull;
  if (cols) {
    if (ncols < 1 || ncols > gel::kOutputColumns)
      return fail(GEL_ERR_ARG, "gel_output_table_batch: ncols = " + std::to_string(ncols) + " outside 1 .. " + std::to_string(gel::kOutputColumns));
    mask = 0;
    for (int k = 0; k < ncols; k++) {
      if (cols[k] < 0 || cols[k] >= gel::kOutputColumns)
        return fail(GEL_ERR_ARG, "gel_output_table_batch: column id " + std::to_string(cols[k]) + " out of range (cols[" + std::to_string(k) + "])");
      if (seen[cols[k]])
        return fail(GEL_ERR_ARG, "gel_output_table_batch: column id " + std::to_string(cols[k]) + " repeated (cols[" + std::to_string(k) + "])");
      seen[cols[k]] = true;
      C.col[k] = (int8_t)cols[k];
      mask |= 1ull << cols[k];
    }
    C.ncols = ncols;
  }
  // what the selected columns need: downrange (5) Vincenty, 7 .. 12 the orbital elements, 3 / 4 the impact point (gel_output_row.h kRow*)
  C.parts = ((mask >> 5 & 1) ? 1u : 0u) | ((mask >> 7 & 0x3f) ? 2u : 0u) | ((mask >> 3 & 3) ? 4u : 0u);
  return GEL_OK;
}

// the launches of one call on the handle's stream
static int outbatch_enqueue(gel_problem* p, const gel::OutBatchArgs& A, const gel_wind_ensemble* ens, double* d_out, double* d_env,
                            double* d_peaks) {
  hipStream_t s = p->stream.get();
  const gel::EnsDev E = ens_dev(ens, 0);
  const size_t lds = gel::outbatch_lds_bytes(p->dev.Kw, p->dev.Kc);
  if (int rc = check_launch_lds("gel_output_table_batch", lds, gel::staged_table_doubles(p->dev.Kw, p->dev.Kc),
                                gel::padded_table_doubles(p->dev.Kw, p->dev.Kc), true))
    return rc;
  if (A.B > 0 && (d_out || d_peaks)) HIPCHK(gel::launch_outbatch_rows(p->dev, A, E, d_out, d_peaks, s));
  if (d_env) {
    const size_t need = gel::outbatch_ws_doubles(A.B, p->dims.M, A.cols.ncols);
    GROW_AFTER_DRAIN(p, p->d_outws, need);
    HIPCHK(gel::launch_outbatch_env(p->dev, A, E, A.B > 0 ? d_out : nullptr, p->d_outws.get(), d_env, s));
  }
  return GEL_OK;
}

int gel_output_table_batch_ensemble_device(gel_problem* p, int32_t B, const double* d_x, const double* d_tx, const double* d_disp,
                                           gel_wind_ensemble* ens, double launch_lat_deg, double launch_lon_deg, int32_t ncols,
                                           const int32_t* cols, double* d_out, double* d_env, double* d_peaks) {
  gel::OutBatchArgs A{};
  if (int rc = outbatch_check(p, B, d_x, ncols, cols, d_out, d_env, d_peaks, A.cols)) return rc;
  if (int rc = ens_check("gel_output_table_batch_ensemble", ens, p, B)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  A.B = B; A.x = d_x; A.tx = d_tx; A.disp = d_disp; A.lat0 = launch_lat_deg; A.lon0 = launch_lon_deg;
  return outbatch_enqueue(p, A, ens, d_out, d_env, d_peaks);
}

int gel_output_table_batch_device(gel_problem* p, int32_t B, const double* d_x, const double* d_tx, const double* d_disp,
                                  double launch_lat_deg, double launch_lon_deg, int32_t ncols, const int32_t* cols, double* d_out,
                                  double* d_env, double* d_peaks) {
  return gel_output_table_batch_ensemble_device(p, B, d_x, d_tx, d_disp, nullptr, launch_lat_deg, launch_lon_deg, ncols, cols, d_out, d_env,
                                                d_peaks);
}

int gel_output_table_batch_ensemble(gel_problem* p, int32_t B, const double* x, const double* tx, const double* disp,
                                    gel_wind_ensemble* ens, double launch_lat_deg, double launch_lon_deg, int32_t ncols,
                                    const int32_t* cols, double* out, double* env, double* peaks) {
  gel::OutBatchArgs A{};
  if (int rc = outbatch_check(p, B, x, ncols, cols, out, env, peaks, A.cols)) return rc;
  if (int rc = ens_check("gel_output_table_batch_ensemble", ens, p, B)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  const size_t M = (size_t)p->dims.M, nc = (size_t)A.cols.ncols, nB = (size_t)B;
  A.B = B; A.lat0 = launch_lat_deg; A.lon0 = launch_lon_deg;
  // (B = 0: x may be NULL; nothing is read)
  return staged_call(p, kStagedNoFlag,
                     {staged_in(B > 0 ? x : nullptr, nB * p->dims.num_vars), staged_in(B > 0 ? tx : nullptr, nB * M),
                      staged_out(out, nB * M * nc), staged_out(env, M * nc * gel::kEnvNStat), staged_out(peaks, nB * nc * gel::kPeakNStat),
                      staged_in(B > 0 ? disp : nullptr, nB * p->dims.S * GEL_PROP_NDISP)},
                     [&](const gel::ProblemDev&, double* const* a) -> int {
                       A.x = a[0]; A.tx = a[1]; A.disp = a[5];
                       return outbatch_enqueue(p, A, ens, a[2], a[3], a[4]);
                     });
}

int gel_output_table_batch(gel_problem* p, int32_t B, const double* x, const double* tx, const double* disp, double launch_lat_deg,
                           double launch_lon_deg, int32_t ncols, const int32_t* cols, double* out, double* env, double* peaks) {
  return gel_output_table_batch_ensemble(p, B, x, tx, disp, nullptr, launch_lat_deg, launch_lon_deg, ncols, cols, out, env, peaks);
}

// ------------- exact batched quantiles over the vectors of a batch -------------
// the argument checks of both forms, before the device check
static int quant_check(gel_problem* p, int32_t B, int64_t W, int64_t ld, const void* src, int32_t nq, const double* probs, const void* q) {
  if (!p) return fail(GEL_ERR_ARG, "gel_batch_quantiles: null handle");
  if (B < 0 || W < 0) return fail(GEL_ERR_ARG, "gel_batch_quantiles: B < 0 or W < 0");
  if (ld < W) return fail(GEL_ERR_ARG, "gel_batch_quantiles: ld = " + std::to_string(ld) + " < W = " + std::to_string(W));
  if (!src && B > 0 && W > 0) return fail(GEL_ERR_ARG, "gel_batch_quantiles: src is NULL with B W > 0");
  if (!q) return fail(GEL_ERR_ARG, "gel_batch_quantiles: q is NULL");
  if (nq < 1 || nq > gel::kQuantMaxQ)
    return fail(GEL_ERR_ARG, "gel_batch_quantiles: nq = " + std::to_string(nq) + " outside 1 .. " + std::to_string(gel::kQuantMaxQ));
  if (!probs) return fail(GEL_ERR_ARG, "gel_batch_quantiles: probs is NULL");
  for (int j = 0; j < nq; j++)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0))   // NaN fails both comparisons
      return fail(GEL_ERR_ARG, "gel_batch_quantiles: probs[" + std::to_string(j) + "] is not a number in [0, 1]");
  return GEL_OK;
}

// the launches of one call on the handle's stream: the source is walked in slabs of columns, each through the same workspace
static int quant_enqueue(gel_problem* p, int32_t B, int64_t W, int64_t ld, const double* d_src, int32_t nq, const double* probs, double* d_q,
                         double* d_count, double* d_who) {
  const int T = 2 * nq;
  p->quant_targets = W * T;
  if (W == 0) return GEL_OK;
  hipStream_t s = p->stream.get();
  const int64_t slab = std::min<int64_t>(gel::quant_slab_cols(T), W);
  const gel::QuantLayout L = gel::quant_layout(slab, T);
  GROW_AFTER_DRAIN(p, p->d_quantws, L.bytes);
  char* ws = p->d_quantws.get();
  HIPCHK(hipMemsetAsync(ws, 0, 256, s));
  gel::QuantArgs A{};
  A.B = B; A.nq = nq; A.T = T; A.ld = ld;
  A.src = reinterpret_cast<const unsigned long long*>(d_src);
  for (int j = 0; j < nq; j++) A.probs[j] = probs[j];
  A.q = d_q; A.count = d_count; A.who = d_who;
  A.counters = reinterpret_cast<unsigned long long*>(ws + L.counters);
  A.col = reinterpret_cast<gel::QuantCol*>(ws + L.col);
  A.hist = reinterpret_cast<uint32_t*>(ws + L.hist);
  A.tgt = reinterpret_cast<gel::QuantTarget*>(ws + L.tgt);
  A.cand = reinterpret_cast<unsigned long long*>(ws + L.cand);
  for (int64_t w0 = 0; w0 < W; w0 += slab) {
    A.w0 = w0;
    A.wn = (int32_t)std::min<int64_t>(slab, W - w0);
    A.chunk = (int32_t)gel::quant_chunk(B, A.wn);
    HIPCHK(gel::launch_quant_slab(A, s));
  }
  return GEL_OK;
}

int gel_batch_quantiles_device(gel_problem* p, int32_t B, int64_t W, int64_t ld, const double* d_src, int32_t nq, const double* probs,
                               double* d_q, double* d_count, double* d_who) {
  if (int rc = quant_check(p, B, W, ld, d_src, nq, probs, d_q)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  return quant_enqueue(p, B, W, ld, d_src, nq, probs, d_q, d_count, d_who);
}

int gel_batch_quantiles(gel_problem* p, int32_t B, int64_t W, int64_t ld, const double* src, int32_t nq, const double* probs, double* q,
                        double* count, double* who) {
  if (int rc = quant_check(p, B, W, ld, src, nq, probs, q)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  // the rows are staged as they lie, [B][ld] up to the last column read: the view stays a view
  const size_t ns = (B > 0 && W > 0) ? (size_t)(B - 1) * (size_t)ld + (size_t)W : 0, no = (size_t)W * nq * 2;
  return staged_call(p, kStagedNoFlag, {staged_in(ns ? src : nullptr, ns), staged_out(q, no), staged_out(count, (size_t)W), staged_out(who, no)},
                     [&](const gel::ProblemDev&, double* const* a) -> int {
                       return quant_enqueue(p, B, W, ld, a[0], nq, probs, a[1], a[2], a[3]);
                     });
}

int gel_batch_quantiles_info(const gel_problem* p, int32_t B, int64_t W, int32_t nq, gel_quantiles_info* info) {
  if (!p || !info || B < 0 || W < 0 || nq < 1 || nq > gel::kQuantMaxQ) return fail(GEL_ERR_ARG, "gel_batch_quantiles_info: bad argument");
  const int T = 2 * nq;
  const int64_t slab = gel::quant_slab_cols(T), used = std::min<int64_t>(slab, W);
  info->bins = gel::kQuantBins;
  info->cap = gel::kQuantCap;
  info->chunk = gel::quant_chunk(B, used);
  info->slab_cols = slab;
  info->workspace_bytes = W > 0 ? (int64_t)gel::quant_layout(used, T).bytes : 0;
  info->workspace_cap_bytes = (int64_t)gel::kQuantWsCap;
  info->passes = B > 0 && W > 0 ? 3 : 0;
  info->slabs = W > 0 ? (W + slab - 1) / slab : 0;
  return GEL_OK;
}

int gel_batch_quantiles_last(gel_problem* p, int64_t* stats) {
  if (!p || !stats) return fail(GEL_ERR_ARG, "gel_batch_quantiles_last: null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  unsigned long long c[4] = {0, 0, 0, 0};
  HIPCHK(hipStreamSynchronize(p->stream.get()));
  if (p->d_quantws.get()) HIPCHK(hipMemcpy(c, p->d_quantws.get(), sizeof(c), hipMemcpyDeviceToHost));
  stats[0] = p->quant_targets;
  for (int k = 1; k < 4; k++) stats[k] = p->quant_targets ? (int64_t)c[k] : 0;
  return GEL_OK;
}

// ------------- batched co-moments over the vectors of a batch -------------
// the argument checks of both forms, before the device check
static int comom_check(const gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const void* a, int64_t Wb, int64_t incb,
                       int64_t ldb, const void* b, const void* C, const void* stat_b, const void* info) {
  if (!p) return fail(GEL_ERR_ARG, "gel_batch_comoments: null handle");
  if (B < 0) return fail(GEL_ERR_ARG, "gel_batch_comoments: B < 0");
  if (Wa < 0 || (b && Wb < 0)) return fail(GEL_ERR_ARG, "gel_batch_comoments: W < 0");
  if (inca < 1 || (b && incb < 1)) return fail(GEL_ERR_ARG, "gel_batch_comoments: inc < 1");
  const auto too_small = [](int64_t W, int64_t inc, int64_t ld) { return W > 0 && (ld < 1 || (W - 1) > (ld - 1) / inc); };   // ld < (W - 1) inc + 1
  if (too_small(Wa, inca, lda)) return fail(GEL_ERR_ARG, "gel_batch_comoments: lda = " + std::to_string(lda) + " < (Wa - 1) inca + 1");
  if (b && too_small(Wb, incb, ldb)) return fail(GEL_ERR_ARG, "gel_batch_comoments: ldb = " + std::to_string(ldb) + " < (Wb - 1) incb + 1");
  if (!a && B > 0 && Wa > 0) return fail(GEL_ERR_ARG, "gel_batch_comoments: a is NULL with B Wa > 0");
  if (!info) return fail(GEL_ERR_ARG, "gel_batch_comoments: info is NULL");
  if (!b && stat_b) return fail(GEL_ERR_ARG, "gel_batch_comoments: stat_b given in the self form (b is NULL)");
  const int64_t wb = b ? Wb : Wa;
  if (!C && Wa > 0 && wb > 0) return fail(GEL_ERR_ARG, "gel_batch_comoments: C is NULL with Wa Wb > 0");
  return GEL_OK;
}

// columns per slab at the most: GEL_COMOM_SLAB (b columns) and GEL_COMOM_SLAB_ROWS (a columns), measurement switches read per call;
// 0 / unset = what the cap holds.  The results do not depend on them.
static int64_t comom_max_slab(const char* name) {
  if (const char* e = getenv(name)) {
    const long long w = atoll(e);
    if (w >= 1) return w;
  }
  return 0;
}
static int comom_plan(int32_t B, int64_t Wa, int64_t Wb, gel::ComSlabs& S) {
  S = gel::com_slabs(B, Wa, Wb, comom_max_slab("GEL_COMOM_SLAB_ROWS"), comom_max_slab("GEL_COMOM_SLAB"));
  if (!S.ok)
    return fail(GEL_ERR_ARG, "gel_batch_comoments: B = " + std::to_string(B) + " vectors of " + std::to_string(Wa) + " + " + std::to_string(Wb) +
                                 " columns leave no room for one tile of pairs in the 256 MiB workspace: fewer columns or vectors per call");
  return GEL_OK;
}

// the launches of one call on the handle's stream: mask and info, the pairs in slabs through the same workspace, the statistics
static int comom_enqueue(gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const double* d_a, int64_t Wb, int64_t incb,
                         int64_t ldb, const double* d_b, bool self, double* d_C, double* d_stat_a, double* d_stat_b, double* d_info) {
  gel::ComSlabs S;
  if (int rc = comom_plan(B, Wa, Wb, S)) return rc;
  hipStream_t s = p->stream.get();
  const gel::ComLayout L = gel::com_layout(B, Wa, S.an, S.bn);
  GROW_AFTER_DRAIN(p, p->d_comws, L.bytes);
  char* ws = p->d_comws.get();
  gel::ComArgs A{};
  A.B = B; A.self = self ? 1 : 0;
  A.Wa = Wa; A.inca = inca; A.lda = lda; A.a = d_a;
  A.Wb = Wb; A.incb = incb; A.ldb = ldb; A.b = d_b;
  A.C = d_C; A.stat_a = d_stat_a; A.stat_b = d_stat_b; A.info = d_info;
  A.cnt = reinterpret_cast<int32_t*>(ws + L.cnt);
  A.fe = reinterpret_cast<int32_t*>(ws + L.fe);
  A.mask = reinterpret_cast<unsigned char*>(ws + L.mask);
  A.sa = reinterpret_cast<double*>(ws + L.sa);
  A.sb = reinterpret_cast<double*>(ws + L.sb);
  A.cp = reinterpret_cast<double*>(ws + L.cp);
  HIPCHK(gel::launch_comom_mask(A, s));
  if (Wa == 0 || Wb == 0) return GEL_OK;
  for (int64_t a0 = 0; a0 < Wa; a0 += S.an)
    for (int64_t b0 = 0; b0 < Wb; b0 += S.bn) {
      const int64_t bn = std::min<int64_t>(S.bn, Wb - b0);
      HIPCHK(gel::launch_comom_slab(A, a0, std::min<int64_t>(S.an, Wa - a0), b0, bn, s));
      if (a0 == 0 && d_stat_b) HIPCHK(gel::launch_comom_stats(A, bn, A.sb, d_stat_b + 2 * b0, s));   // the slab's b columns, before the next slab
    }
  HIPCHK(gel::launch_comom_stats(A, Wa, A.sa, d_stat_a, s));
  return GEL_OK;
}

int gel_batch_comoments_device(gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const double* d_a, int64_t Wb, int64_t incb,
                               int64_t ldb, const double* d_b, double* d_C, double* d_stat_a, double* d_stat_b, double* d_info) {
  if (int rc = comom_check(p, B, Wa, inca, lda, d_a, Wb, incb, ldb, d_b, d_C, d_stat_b, d_info)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  const bool self = !d_b;
  if (self) return comom_enqueue(p, B, Wa, inca, lda, d_a, Wa, inca, lda, d_a, true, d_C, d_stat_a, nullptr, d_info);
  return comom_enqueue(p, B, Wa, inca, lda, d_a, Wb, incb, ldb, d_b, false, d_C, d_stat_a, d_stat_b, d_info);
}

int gel_batch_comoments(gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const double* a, int64_t Wb, int64_t incb,
                        int64_t ldb, const double* b, double* C, double* stat_a, double* stat_b, double* info) {
  if (int rc = comom_check(p, B, Wa, inca, lda, a, Wb, incb, ldb, b, C, stat_b, info)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  const bool self = !b;
  if (self) { Wb = Wa; incb = inca; ldb = lda; }
  // the rows are staged as they lie, up to the last entry read: the views stay views
  const auto span = [&](int64_t W, int64_t inc, int64_t ld) { return (B > 0 && W > 0) ? (size_t)(B - 1) * (size_t)ld + (size_t)(W - 1) * (size_t)inc + 1 : 0; };
  const size_t na = span(Wa, inca, lda), nb = self ? 0 : span(Wb, incb, ldb);
  const bool pairs = Wa > 0 && Wb > 0;   // Wa = 0 or Wb = 0: info only, nothing else is written
  return staged_call(p, kStagedNoFlag,
                     {staged_in(na ? a : nullptr, na), staged_in(nb ? b : nullptr, nb), staged_out(pairs ? C : nullptr, (size_t)Wa * (size_t)Wb),
                      staged_out(pairs ? stat_a : nullptr, (size_t)Wa * 2), staged_out(pairs && !self ? stat_b : nullptr, (size_t)Wb * 2),
                      staged_out(info, 2)},
                     [&](const gel::ProblemDev&, double* const* d) -> int {
                       return comom_enqueue(p, B, Wa, inca, lda, d[0], Wb, incb, ldb, self ? d[0] : d[1], self, d[2], d[3], d[4], d[5]);
                     });
}

int gel_batch_comoments_info(const gel_problem* p, int32_t B, int64_t Wa, int64_t Wb, int32_t self, gel_comoments_info* out) {
  if (!p || !out || B < 0 || Wa < 0 || (!self && Wb < 0)) return fail(GEL_ERR_ARG, "gel_batch_comoments_info: bad argument");
  if (self) Wb = Wa;
  gel::ComSlabs S;
  if (int rc = comom_plan(B, Wa, Wb, S)) return rc;
  const bool pairs = Wa > 0 && Wb > 0;
  out->block = gel::kComBlock;
  out->tile_a = gel::kComTileA;
  out->tile_b = gel::kComTileB;
  out->slab_rows = S.an;
  out->slab_cols = S.bn;
  out->slabs = pairs ? ((Wa + S.an - 1) / S.an) * ((Wb + S.bn - 1) / S.bn) : 0;
  out->workspace_bytes = (int64_t)gel::com_layout(B, Wa, S.an, S.bn).bytes;
  out->workspace_cap_bytes = (int64_t)gel::kComWsCap;
  // reads of a source entry: the mask pass, then once per tile of the other view's columns (from the caches after the first)
  out->passes_a = B > 0 && Wa > 0 ? 1 + (pairs ? (Wb + gel::kComTileB - 1) / gel::kComTileB : 0) : 0;
  out->passes_b = B > 0 && Wb > 0 && !self ? 1 + (pairs ? (Wa + gel::kComTileA - 1) / gel::kComTileA : 0) : 0;
  return GEL_OK;
}

}  // extern "C"
