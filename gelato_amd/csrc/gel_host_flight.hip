// gel_host_flight.hip -- the flown trajectory: the propagation plan and gel_propagate* (DESIGN.md 3.14), the wind ensemble
// (gel_wind_ensemble_*; 3.19), the tangent-linear flight (3.20), the adjoint flight (3.21), both under an ensemble (3.22) and with
// the wind table's rows as a direction or a gradient (3.23), and their _info calls.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gel_prop.h"
#include "gel_proptan.h"
#include "gel_propadj.h"
#include "gel_host_handle.h"

using namespace gelhost;

namespace gelhost {

// an evaluation call's ensemble: of the same source handle, and assigned exactly the call's B vectors
int ens_check(const char* what, const gel_wind_ensemble* ens, const gel_problem* src, int32_t B) {
  if (!ens) return GEL_OK;
  if (ens->src != src) return fail(GEL_ERR_ARG, std::string(what) + ": the wind ensemble belongs to another handle");
  if (ens->assigned != B)
    return fail(GEL_ERR_ARG, std::string(what) + ": the wind ensemble is assigned " +
                                 (ens->assigned < 0 ? std::string("no vectors yet") : std::to_string(ens->assigned) + " vectors") +
                                 ", the call has B = " + std::to_string(B) + " (gel_wind_ensemble_assign)");
  return GEL_OK;
}

}  // namespace gelhost

extern "C" {

// ------------- batched explicit propagation of the sections with RK4: the shooting check -------------
// A plan = per phase the stage points, the step of every node interval and the matrix that samples the control polynomial at the
// stage points (the interpolation plan's builder: the same bits), row-major on the host (gel_prop_matrices), transposed on the
// device (gel_prop.h).  It owns its tables and the control samples' workspace and refers to the source handle for the device,
// the stream, the non-finite flag and the arena of the host-buffer form (staged_call): it is destroyed before that handle.
struct gel_prop_plan {
  gel_problem* src = nullptr;
  int32_t flags = 0;
  gel::PropDev dev{};
  std::vector<gel::PropPhaseDev> ph;
  std::vector<double> pts, Wu;    // per phase pts [Pp] at poff[s], Wu [Pp][n] row-major at woff[s]
  std::vector<size_t> poff, woff;
  std::vector<int32_t> cp;        // copy_u [Pp] per phase at ph[s].cu (the device's array as it is)
  int64_t total_pts = 0;          // sum over all phases of Pp
  int64_t sampled_pts = 0;        // sum over the free-attitude phases of Pp: the workspace's rows
  int64_t lane_steps = 0;         // RK4 steps of the longest lane
  int n_max_sampled = 0;
  DeviceArray<double> d_mat, d_ws;
  DeviceArray<int32_t> d_cp, d_seg;
  DeviceArray<gel::PropPhaseDev> d_ph;
};

static constexpr int64_t kPropWsBytes = 1LL << 30;       // the control samples' workspace never exceeds this
static constexpr int64_t kPropMaxSlab = 1 << 20;         // vectors per slab at the most
static constexpr int64_t kPropMaxMatDoubles = 1LL << 27; // sum over phases of Pp n: the plan's matrices stay below 1 GB

// doubles per vector of a flight call's arrays: the decision vector (nv), the flown states (ny), the dispersions (nd)
struct PropStrides { size_t nv, ny, nd; };
static PropStrides prop_strides(const gel_problem* p) {
  return {(size_t)p->dims.num_vars, (size_t)11 * p->dims.M, (size_t)p->dims.S * GEL_PROP_NDISP};
}

// GEL_PROP_SLAB (measurement switch, read per call, rounded up to a multiple of 64; a value above the cap vs is ignored) or vs
static int64_t slab_or_env(int64_t vs) {
  if (const char* e = getenv("GEL_PROP_SLAB")) {
    const long long w = (atoll(e) + 63) / 64 * 64;
    if (w >= 64 && w <= vs) vs = w;
  }
  return vs;
}

// Vectors per slab of a call (what gel_prop_plan_info reports): as many as the workspace cap holds, a multiple of 64; or
// GEL_PROP_SLAB (slab_or_env).  The results do not depend on it.
static int64_t prop_slab(const gel_prop_plan* pl) {
  const int64_t per_vec = 16 * pl->sampled_pts;
  int64_t vs = per_vec ? std::min<int64_t>(kPropMaxSlab, kPropWsBytes / per_vec / 64 * 64) : kPropMaxSlab;
  if (vs < 64) vs = 64;   // (a host-only handle's plan may hold more stage points than a device handle's: creation refuses those there)
  return slab_or_env(vs);
}

int gel_prop_plan_create(gel_problem* src, const int32_t* steps, int32_t flags, gel_prop_plan** out) {
  if (!src || !steps || !out || (flags & ~(GEL_PROP_RESTART_NODE | GEL_PROP_CHAIN))) return fail(GEL_ERR_ARG, "bad argument");
  if ((flags & GEL_PROP_RESTART_NODE) && (flags & GEL_PROP_CHAIN))
    return fail(GEL_ERR_ARG, "propagation plan: GEL_PROP_CHAIN and GEL_PROP_RESTART_NODE exclude each other");
  const int S = src->dims.S;
  const bool chain = (flags & GEL_PROP_CHAIN) != 0;
  int64_t mat_doubles = 0, chain_steps = 0;
  for (int s = 0; s < S; s++) {
    if (steps[s] < 1) return fail(GEL_ERR_ARG, "propagation plan: steps < 1");
    if ((int64_t)steps[s] * src->ph[s].n > gel::kPropMaxLaneSteps)
      return fail(GEL_ERR_ARG, "propagation plan: steps[s] n_s exceeds 2^20 RK4 steps in one section");
    mat_doubles += (2 * (int64_t)steps[s] * src->ph[s].n + 1) * src->ph[s].n;
    chain_steps += (int64_t)steps[s] * src->ph[s].n;   // (at most S 2^20: no overflow)
  }
  if (chain && chain_steps > gel::kPropMaxLaneSteps)
    return fail(GEL_ERR_ARG, "propagation plan: the sum of steps[s] n_s exceeds 2^20 RK4 steps in one chained flight");
  if (mat_doubles > kPropMaxMatDoubles) return fail(GEL_ERR_ARG, "propagation plan: the control matrices (sum of (2 k n + 1) n doubles) exceed 1 GB");
  std::unique_ptr<gel_prop_plan> pl(new gel_prop_plan);
  pl->src = src;
  pl->flags = flags;
  const bool restart = (flags & GEL_PROP_RESTART_NODE) != 0;
  pl->ph.resize(S);
  pl->poff.resize(S);
  pl->woff.resize(S);
  std::vector<double> matT;      // the device's table: per phase sig | hs | WuT (sampled phases only)
  std::vector<int32_t> seg_phase;
  for (int s = 0; s < S; s++) {
    const HostPhase& h = src->ph[s];
    const int n = h.n, k = steps[s];
    const int64_t Pp = 2 * (int64_t)k * n + 1;
    gel::PropPhaseDev& q = pl->ph[s];
    q.n = n; q.k = k; q.sampled = h.hold ? 0 : 1; q.pad = 0;
    q.ntile = q.sampled ? (int32_t)((Pp + gel::kPropSampleThreads - 1) / gel::kPropSampleThreads) : 0;
    q.seg0 = (int32_t)seg_phase.size();
    seg_phase.insert(seg_phase.end(), restart ? n : 1, s);
    q.pt0 = pl->sampled_pts;
    if (q.sampled) { pl->sampled_pts += Pp; pl->n_max_sampled = std::max(pl->n_max_sampled, n); }
    pl->total_pts += Pp;
    pl->lane_steps = chain ? chain_steps : std::max<int64_t>(pl->lane_steps, restart ? k : (int64_t)k * n);
    std::vector<ld> tx(n + 1), tc(n);
    tx[0] = -1.0L;
    for (int j = 0; j < n; j++) tx[j + 1] = tc[j] = (ld)h.tau[j];
    // stage points: a point on a node is the node's fp64 value itself
    pl->poff[s] = pl->pts.size();
    std::vector<double> hs(n);
    for (int j = 0; j < n; j++) {
      hs[j] = ((double)tx[j + 1] - (double)tx[j]) / (double)k;
      for (int m = (j ? 1 : 0); m <= 2 * k; m++)
        pl->pts.push_back(m == 0 ? (double)tx[j] : m == 2 * k ? (double)tx[j + 1]
                                                             : (double)(tx[j] + (tx[j + 1] - tx[j]) * (ld)m / (ld)(2 * k)));
    }
    const double* z = pl->pts.data() + pl->poff[s];
    const std::vector<ld> wc = bary_weights(tc);
    pl->woff[s] = pl->Wu.size();
    q.cu = (int64_t)pl->cp.size();
    std::vector<ld> row(n);
    for (int64_t l = 0; l < Pp; l++) {
      lagrange_row(tc, wc, (ld)z[l], row.data());
      int32_t c = -1;
      for (int j = 0; j < n; j++) {
        pl->Wu.push_back((double)row[j]);
        if ((double)tc[j] == z[l]) c = j;
      }
      pl->cp.push_back(c);
    }
    q.sg = (int64_t)matT.size();
    matT.insert(matT.end(), z, z + Pp);
    q.hs = (int64_t)matT.size();
    matT.insert(matT.end(), hs.begin(), hs.end());
    q.wu = (int64_t)matT.size();
    if (q.sampled) {
      const double* W = pl->Wu.data() + pl->woff[s];
      for (int j = 0; j < n; j++)
        for (int64_t l = 0; l < Pp; l++) matT.push_back(W[(size_t)l * n + j]);
    }
  }
  gel::PropDev& d = pl->dev;
  d.S = S; d.restart = restart ? 1 : 0; d.nseg = (int32_t)seg_phase.size(); d.chain = chain ? 1 : 0;
  d.vp = src->uv / src->up;
  if (src->device != GEL_DEVICE_NONE) {
    if (gel::prop_sample_lds_bytes(pl->n_max_sampled) > gel::kPropMaxLds)
      return fail(GEL_ERR_ARG, "propagation plan: a free-attitude phase's controls (8 n doubles) do not fit a workgroup's LDS (n > 1024)");
    if (64 * 16 * pl->sampled_pts > kPropWsBytes)
      return fail(GEL_ERR_ARG, "propagation plan: the control samples of 64 vectors (16 bytes per stage point) exceed the 1 GB workspace");
    HIPCHK(hipSetDevice(src->device));
    HIPCHK(pl->d_mat.upload(matT));
    HIPCHK(pl->d_cp.upload(pl->cp));
    HIPCHK(pl->d_seg.upload(seg_phase));
    HIPCHK(pl->d_ph.upload(pl->ph));
    d.ph = pl->d_ph.get(); d.seg_phase = pl->d_seg.get(); d.mat = pl->d_mat.get(); d.cp = pl->d_cp.get();
  }
  *out = pl.release();
  return GEL_OK;
}

int gel_prop_plan_destroy(gel_prop_plan* plan) {
  if (!plan) return GEL_OK;
  if (plan->src->device != GEL_DEVICE_NONE) {
    hipSetDevice(plan->src->device);
    (void)drain(plan->src);   // a device call in flight still reads the plan's tables and workspace
  }
  delete plan;
  return GEL_OK;
}

int gel_prop_plan_info(const gel_prop_plan* plan, int64_t* info) {
  if (!plan || !info) return fail(GEL_ERR_ARG, "null argument");
  info[0] = plan->dev.S; info[1] = plan->flags; info[2] = plan->total_pts; info[3] = plan->lane_steps;
  info[4] = 16 * plan->sampled_pts; info[5] = prop_slab(plan);
  return GEL_OK;
}

int gel_prop_matrices(const gel_prop_plan* plan, int32_t phase, double* pts, double* Wu, int32_t* copy_u) {
  if (!plan || phase < 0 || phase >= plan->dev.S) return fail(GEL_ERR_ARG, "bad argument");
  const gel::PropPhaseDev& q = plan->ph[phase];
  const size_t Pp = 2 * (size_t)q.k * q.n + 1;
  if (pts) std::memcpy(pts, plan->pts.data() + plan->poff[phase], Pp * 8);
  if (Wu) std::memcpy(Wu, plan->Wu.data() + plan->woff[phase], Pp * q.n * 8);
  if (copy_u) std::memcpy(copy_u, plan->cp.data() + q.cu, Pp * 4);
  return GEL_OK;
}

// ------------- wind ensemble of a Monte-Carlo batch (struct gel_wind_ensemble and ens_dev: gel_host_handle.h) -------------
int gel_wind_ensemble_create(gel_problem* src, int32_t E, int32_t Kw, const double* tables, gel_wind_ensemble** out) {
  if (!src || !out) return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: null handle or result pointer");
  if (E < 1) return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: E = " + std::to_string(E) + " < 1");
  if (Kw < 2) return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: Kw = " + std::to_string(Kw) + " < 2 (wind and CA tables need at least two rows)");
  if (Kw > gel::kEnsMaxRows) return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: Kw = " + std::to_string(Kw) + " exceeds 2^20 rows");
  const int64_t stride = 5 * (int64_t)Kw - 2;
  if ((int64_t)E * stride > gel::kEnsMaxDoubles)
    return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: E (5 Kw - 2) = " + std::to_string((int64_t)E * stride) + " doubles exceed 2^27 (1 GB)");
  if (!tables) return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: tables is NULL");
  const double ca2[4] = {0.0, 0.0, 1.0, 0.0};   // (check_tables looks at both tables: a valid two-row CA table beside the member)
  for (int e = 0; e < E; e++)
    if (const char* bad = gel::check_tables(tables + (size_t)e * 3 * (size_t)Kw, Kw, ca2, 2))
      return fail(GEL_ERR_ARG, "gel_wind_ensemble_create: member " + std::to_string(e) + ": " + bad);
  std::unique_ptr<gel_wind_ensemble> en(new gel_wind_ensemble);
  en->src = src; en->E = E; en->Kw = Kw; en->stride = stride;
  en->staged.reserve((size_t)E * (size_t)stride);
  for (int e = 0; e < E; e++) {
    std::vector<double> slopes;
    gel::append_rows_and_slopes(en->staged, slopes, tables + (size_t)e * 3 * (size_t)Kw, Kw, 3);
    en->staged.insert(en->staged.end(), slopes.begin(), slopes.end());
  }
  if (src->device != GEL_DEVICE_NONE) {
    HIPCHK(hipSetDevice(src->device));
    HIPCHK(en->d_tables.upload(en->staged));
  }
  *out = en.release();
  return GEL_OK;
}

int gel_wind_ensemble_destroy(gel_wind_ensemble* ens) {
  if (!ens) return GEL_OK;
  if (ens->src->device != GEL_DEVICE_NONE) {
    hipSetDevice(ens->src->device);
    (void)drain(ens->src);   // a device call in flight still reads the members and the assignment
  }
  delete ens;
  return GEL_OK;
}

int gel_wind_ensemble_info(const gel_wind_ensemble* ens, int64_t* info) {
  if (!ens || !info) return fail(GEL_ERR_ARG, "null argument");
  info[0] = ens->E; info[1] = ens->Kw; info[2] = ens->stride;
  info[3] = (int64_t)(ens->d_tables.capacity() * sizeof(double) + ens->d_member.capacity() * sizeof(int32_t));
  info[4] = ens->assigned;
  return GEL_OK;
}

int gel_wind_ensemble_member(const gel_wind_ensemble* ens, int32_t e, double* staged) {
  if (!ens || !staged) return fail(GEL_ERR_ARG, "null argument");
  if (e < 0 || e >= ens->E) return fail(GEL_ERR_ARG, "gel_wind_ensemble_member: member " + std::to_string(e) + " outside 0 .. " + std::to_string(ens->E - 1));
  std::memcpy(staged, ens->staged.data() + (size_t)e * (size_t)ens->stride, (size_t)ens->stride * 8);
  return GEL_OK;
}

int gel_wind_ensemble_assign(gel_wind_ensemble* ens, int32_t B, const int32_t* member) {
  if (!ens) return fail(GEL_ERR_ARG, "gel_wind_ensemble_assign: null ensemble");
  if (B < 0) return fail(GEL_ERR_ARG, "gel_wind_ensemble_assign: B < 0");
  if (B > 0 && !member) return fail(GEL_ERR_ARG, "gel_wind_ensemble_assign: member is NULL with B > 0");
  for (int32_t b = 0; b < B; b++)
    if (member[b] < -1 || member[b] >= ens->E)
      return fail(GEL_ERR_ARG, "gel_wind_ensemble_assign: member[" + std::to_string(b) + "] = " + std::to_string(member[b]) + " outside -1 .. " +
                                   std::to_string(ens->E - 1));
  if (ens->src->device != GEL_DEVICE_NONE) {
    HIPCHK(hipSetDevice(ens->src->device));
    HIPCHK(drain(ens->src));   // a call in flight still reads the old assignment
    ens->assigned = -1;        // (a failed upload leaves no assignment)
    HIPCHK(ens->d_member.upload(member, (size_t)B));
  }
  ens->assigned = B;
  return GEL_OK;
}

// the launches of one call on stream s: slab after slab the control samples and the integration, then err of all B vectors
static int prop_enqueue(gel_prop_plan* plan, int32_t B, const double* d_x, double* d_y, double* d_err, const double* d_disp,
                        const gel_wind_ensemble* ens, hipStream_t s) {
  gel_problem* p = plan->src;
  const int64_t vs = prop_slab(plan), ldv = std::min<int64_t>(vs, ((int64_t)B + 63) / 64 * 64);
  const size_t need = (size_t)ldv * 2 * (size_t)plan->sampled_pts;
  GROW_AFTER_DRAIN(p, plan->d_ws, need);
  const auto [nv, ny, nd] = prop_strides(p);
  for (int64_t v0 = 0; v0 < B; v0 += vs) {
    const int nb = (int)std::min<int64_t>(vs, B - v0);
    HIPCHK(gel::launch_prop_slab(p->dev, plan->dev, plan->ph.data(), plan->n_max_sampled, nb, d_x + (size_t)v0 * nv,
                                 d_y + (size_t)v0 * ny, plan->d_ws.get(), ldv, d_disp ? d_disp + (size_t)v0 * nd : nullptr,
                                 ens_dev(ens, v0), s));
  }
  if (d_err) HIPCHK(gel::launch_prop_err(p->dev, plan->dev, B, d_x, d_y, d_err, s));
  return GEL_OK;
}

int gel_propagate_ensemble_device(gel_prop_plan* plan, int32_t B, const double* d_x, const double* d_disp, gel_wind_ensemble* ens,
                                  double* d_y, double* d_err) {
  if (!plan || B < 0 || (B > 0 && (!d_x || !d_y))) return fail(GEL_ERR_ARG, "bad argument");
  gel_problem* p = plan->src;
  if (int rc = ens_check("gel_propagate_ensemble", ens, p, B)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (B == 0) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  return prop_enqueue(plan, B, d_x, d_y, d_err, d_disp, ens, p->stream.get());
}

int gel_propagate_dispersed_device(gel_prop_plan* plan, int32_t B, const double* d_x, const double* d_disp, double* d_y,
                                   double* d_err) {
  return gel_propagate_ensemble_device(plan, B, d_x, d_disp, nullptr, d_y, d_err);
}

int gel_propagate_device(gel_prop_plan* plan, int32_t B, const double* d_x, double* d_y, double* d_err) {
  return gel_propagate_dispersed_device(plan, B, d_x, nullptr, d_y, d_err);
}

int gel_propagate_ensemble(gel_prop_plan* plan, int32_t B, const double* x, const double* disp, gel_wind_ensemble* ens, double* y,
                           double* err) {
  if (!plan || B < 0 || (B > 0 && (!x || !y))) return fail(GEL_ERR_ARG, "bad argument");
  gel_problem* p = plan->src;
  if (int rc = ens_check("gel_propagate_ensemble", ens, p, B)) return rc;
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (B == 0) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  const auto [nv, ny, nd] = prop_strides(p);
  // (the ensemble's members and assignment are resident: the arena holds what it held)
  return staged_call(p, 0, {staged_in(x, (size_t)B * nv), staged_out(y, (size_t)B * ny), staged_out(err, (size_t)B * p->dims.S * 4),
                            staged_in(disp, (size_t)B * nd)},
                     [&](const gel::ProblemDev&, double* const* a) { return prop_enqueue(plan, B, a[0], a[1], a[2], a[3], ens, p->stream.get()); });
}

int gel_propagate_dispersed(gel_prop_plan* plan, int32_t B, const double* x, const double* disp, double* y, double* err) {
  return gel_propagate_ensemble(plan, B, x, disp, nullptr, y, err);
}

int gel_propagate(gel_prop_plan* plan, int32_t B, const double* x, double* y, double* err) {
  return gel_propagate_dispersed(plan, B, x, nullptr, y, err);
}

// ------------- tangent-linear propagation: exact flight sensitivities -------------
// The workspace holds one sample set (16 bytes per sampled stage point) per vector of a slab and one per seed: per lane
// (vector, direction), or per direction when the seeds are shared.  Vectors per slab: as many as the plan's 1 GB cap then holds, a
// multiple of 64, at least 64; GEL_PROP_SLAB as in prop_slab().
static int64_t proptan_slab(const gel_prop_plan* pl, int64_t P, bool shared) {
  const int64_t set = 16 * pl->sampled_pts;
  const int64_t per_vec = shared ? set : set * (1 + P), fixed = shared ? set * ((P + 63) / 64 * 64) : 0;
  int64_t vs = per_vec ? std::min<int64_t>(kPropMaxSlab, std::max<int64_t>(0, kPropWsBytes - fixed) / per_vec / 64 * 64) : kPropMaxSlab;
  vs = std::min<int64_t>(vs, (int64_t)0x7fffffff / P / 64 * 64);   // (a slab's lanes fit an int32)
  if (vs < 64) vs = 64;
  return slab_or_env(vs);
}

// the row count of the wind seeds and of gwind (gel_prop_wind_rows): every table a lane of the call may read fits
static int32_t prop_wind_rows(const gel_prop_plan* plan, const gel_wind_ensemble* ens) {
  return std::max<int32_t>(plan->src->dev.Kw, ens ? ens->Kw : 0);
}

// every refusal that is decided before a buffer is looked at: what is wrong, or null (the run calls name it, gel_prop_tangent_info
// answers all of them with one text)
static const char* proptan_refuse(const gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared) {
  if (!plan) return "null plan";
  if (B < 0) return "B < 0";
  if (P < 1) return "P < 1";
  if ((int64_t)B * P > 0x7fffffffLL) return "B P exceeds 2^31 - 1 lanes";
  if (shared != 0 && shared != 1) return "shared is neither 0 nor 1";
  return nullptr;
}

// wind_call: one of gel_propagate_tangent_wind*, which take a third seed (dwind; NULL in the parents' calls)
static int proptan_check(const char* who, const gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const void* x, const void* dx,
                         const void* ddisp, const void* dwind, bool wind_call, const gel_wind_ensemble* ens, const void* y, const void* dy) {
  const std::string w(who);
  if (const char* why = proptan_refuse(plan, B, P, shared)) return fail(GEL_ERR_ARG, w + ": " + why);
  if (!dx && !ddisp && !dwind)
    return fail(GEL_ERR_ARG, w + (wind_call ? ": all three seeds (dx, ddisp, dwind) are NULL" : ": both seeds (dx, ddisp) are NULL"));
  if (B > 0 && (!x || !y || !dy)) return fail(GEL_ERR_ARG, w + ": x, y or dy is NULL with B > 0");
  if (int rc = ens_check(who, ens, plan->src, B)) return rc;
  if (plan->src->device == GEL_DEVICE_NONE) return fail(GEL_ERR_ARG, w + ": the plan's handle is host-only (GEL_DEVICE_NONE)");
  const int64_t set = 16 * plan->sampled_pts;
  if ((shared ? set * (((int64_t)P + 63) / 64 * 64 + 64) : set * 64 * (1 + (int64_t)P)) > kPropWsBytes)
    return fail(GEL_ERR_ARG, w + ": the control samples of 64 vectors and their seeds exceed the 1 GB workspace");
  return GEL_OK;
}

int gel_prop_tangent_info(const gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, int64_t* info) {
  if (!info || proptan_refuse(plan, B, P, shared)) return fail(GEL_ERR_ARG, "gel_prop_tangent_info: bad argument");
  const int64_t vs = proptan_slab(plan, P, shared != 0);
  info[0] = 16 * plan->sampled_pts;
  info[1] = vs * P;
  info[2] = (B + vs - 1) / vs;
  return GEL_OK;
}

// the launches of one call on stream s, slab after slab: the control samples of the slab's vectors, those of its seeds (the shared
// seeds' once, before the first slab), the integration
static int proptan_enqueue(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x, const double* d_disp,
                           const double* d_dx, const double* d_ddisp, const double* d_dwind, const gel_wind_ensemble* ens, double* d_y,
                           double* d_dy, hipStream_t s) {
  gel_problem* p = plan->src;
  const int32_t Kg = prop_wind_rows(plan, ens);
  const int64_t vs = proptan_slab(plan, P, shared != 0), ldv = std::min<int64_t>(vs, ((int64_t)B + 63) / 64 * 64);
  const int64_t dld = d_dx ? (shared ? ((int64_t)P + 63) / 64 * 64 : ldv * P) : 0;
  const size_t set = 2 * (size_t)plan->sampled_pts, need = (size_t)(ldv + dld) * set;
  GROW_AFTER_DRAIN(p, plan->d_ws, need);
  double* const ws = plan->d_ws.get();
  double* const dws = ws + (size_t)ldv * set;   // the second region: the seeds' samples
  // prop_sample_kernel alone: launch_prop_slab on a copy of the plan's tables that has no segment to integrate
  gel::PropDev sample_only = plan->dev;
  sample_only.chain = 0;
  sample_only.restart = 0;
  sample_only.nseg = 0;
  const auto [nv, ny, nd] = prop_strides(p);
  const gel::EnsDev no_ens{};
  if (d_dx && shared)
    HIPCHK(gel::launch_prop_slab(p->dev, sample_only, plan->ph.data(), plan->n_max_sampled, P, d_dx, nullptr, dws, dld, nullptr, no_ens, s));
  for (int64_t v0 = 0; v0 < B; v0 += vs) {
    const int nb = (int)std::min<int64_t>(vs, B - v0);
    HIPCHK(gel::launch_prop_slab(p->dev, sample_only, plan->ph.data(), plan->n_max_sampled, nb, d_x + (size_t)v0 * nv, nullptr, ws, ldv,
                                 nullptr, no_ens, s));
    const size_t l0 = (size_t)v0 * P;   // the slab's first lane
    if (d_dx && !shared)
      HIPCHK(gel::launch_prop_slab(p->dev, sample_only, plan->ph.data(), plan->n_max_sampled, nb * P, d_dx + l0 * nv, nullptr, dws, dld,
                                   nullptr, no_ens, s));
    gel::PropTanArgs a{};
    a.nb = nb; a.P = P; a.shared = shared;
    a.x = d_x + (size_t)v0 * nv;
    a.disp = d_disp ? d_disp + (size_t)v0 * nd : nullptr;
    a.dx = d_dx ? (shared ? d_dx : d_dx + l0 * nv) : nullptr;
    a.ddisp = d_ddisp ? (shared ? d_ddisp : d_ddisp + l0 * nd) : nullptr;
    a.y = d_y + (size_t)v0 * ny;
    a.dy = d_dy + l0 * ny;
    a.ws = ws; a.dws = dws; a.ld = ldv; a.dld = dld;
    gel::WindSeedDev wd{};   // (the seeds are read where the caller keeps them: no workspace)
    if (d_dwind) { wd.dwind = shared ? d_dwind : d_dwind + l0 * 2 * (size_t)Kg; wd.Kg = Kg; }
    HIPCHK(gel::launch_proptan_slab(p->dev, plan->dev, a, ens_dev(ens, v0), wd, s));
  }
  return GEL_OK;
}

// (the refusals name the entry point the caller used: with an ensemble the _ensemble one)
static int proptan_device(const char* who, gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x, const double* d_disp,
                          const double* d_dx, const double* d_ddisp, gel_wind_ensemble* ens, double* d_y, double* d_dy,
                          const double* d_dwind = nullptr, bool wind_call = false) {
  if (int rc = proptan_check(who, plan, B, P, shared, d_x, d_dx, d_ddisp, d_dwind, wind_call, ens, d_y, d_dy)) return rc;
  if (B == 0) return GEL_OK;
  gel_problem* p = plan->src;
  HIPCHK(hipSetDevice(p->device));
  return proptan_enqueue(plan, B, P, shared, d_x, d_disp, d_dx, d_ddisp, d_dwind, ens, d_y, d_dy, p->stream.get());
}

int gel_propagate_tangent_ensemble_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x, const double* d_disp,
                                          const double* d_dx, const double* d_ddisp, gel_wind_ensemble* ens, double* d_y, double* d_dy) {
  return proptan_device("gel_propagate_tangent_ensemble_device", plan, B, P, shared, d_x, d_disp, d_dx, d_ddisp, ens, d_y, d_dy);
}

int gel_propagate_tangent_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x, const double* d_disp,
                                 const double* d_dx, const double* d_ddisp, double* d_y, double* d_dy) {
  return proptan_device("gel_propagate_tangent_device", plan, B, P, shared, d_x, d_disp, d_dx, d_ddisp, nullptr, d_y, d_dy);
}

static int proptan_host(const char* who, gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp,
                        const double* dx, const double* ddisp, gel_wind_ensemble* ens, double* y, double* dy, const double* dwind = nullptr,
                        bool wind_call = false) {
  if (int rc = proptan_check(who, plan, B, P, shared, x, dx, ddisp, dwind, wind_call, ens, y, dy)) return rc;
  if (B == 0) return GEL_OK;
  gel_problem* p = plan->src;
  HIPCHK(hipSetDevice(p->device));
  const auto [nv, ny, nd] = prop_strides(p);
  const size_t seeds = shared ? (size_t)P : (size_t)B * P;
  // (x, y, disp as gel_propagate_dispersed lays them out; the new buffers behind them; the ensemble's members and assignment are
  // resident: the arena holds what it held)
  return staged_call(p, 0, {staged_in(x, (size_t)B * nv), staged_out(y, (size_t)B * ny), staged_in(disp, (size_t)B * nd),
                            staged_in(dx, seeds * nv), staged_in(ddisp, seeds * nd), staged_out(dy, (size_t)B * P * ny),
                            staged_in(dwind, seeds * 2 * (size_t)prop_wind_rows(plan, ens))},
                     [&](const gel::ProblemDev&, double* const* a) {
                       return proptan_enqueue(plan, B, P, shared, a[0], a[2], a[3], a[4], a[6], ens, a[1], a[5], p->stream.get());
                     });
}

int gel_propagate_tangent_ensemble(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp,
                                   const double* dx, const double* ddisp, gel_wind_ensemble* ens, double* y, double* dy) {
  return proptan_host("gel_propagate_tangent_ensemble", plan, B, P, shared, x, disp, dx, ddisp, ens, y, dy);
}

int gel_propagate_tangent(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp, const double* dx,
                          const double* ddisp, double* y, double* dy) {
  return proptan_host("gel_propagate_tangent", plan, B, P, shared, x, disp, dx, ddisp, nullptr, y, dy);
}

// the wind table's own direction beside dx and ddisp; dwind == NULL: the calls above
int gel_propagate_tangent_wind_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x, const double* d_disp,
                                      const double* d_dx, const double* d_ddisp, const double* d_dwind, gel_wind_ensemble* ens, double* d_y,
                                      double* d_dy) {
  return proptan_device("gel_propagate_tangent_wind_device", plan, B, P, shared, d_x, d_disp, d_dx, d_ddisp, ens, d_y, d_dy, d_dwind, true);
}

int gel_propagate_tangent_wind(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp,
                               const double* dx, const double* ddisp, const double* dwind, gel_wind_ensemble* ens, double* y, double* dy) {
  return proptan_host("gel_propagate_tangent_wind", plan, B, P, shared, x, disp, dx, ddisp, ens, y, dy, dwind, true);
}

int gel_prop_wind_rows(const gel_prop_plan* plan, const gel_wind_ensemble* ens, int32_t* Kg) {
  if (!plan) return fail(GEL_ERR_ARG, "gel_prop_wind_rows: null plan");
  if (!Kg) return fail(GEL_ERR_ARG, "gel_prop_wind_rows: Kg is NULL");
  if (ens && ens->src != plan->src) return fail(GEL_ERR_ARG, "gel_prop_wind_rows: the wind ensemble belongs to another handle");
  *Kg = prop_wind_rows(plan, ens);
  return GEL_OK;
}

// ------------- adjoint flight: gradients of the flown trajectory in one pass -------------
// The workspace holds per vector of a slab one sample set (16 bytes per sampled stage point) and per lane (vector, functional) the
// stage points' control multipliers (as many bytes again), one double per phase (the multiplier of S) and the inner checkpoints of
// one node interval (11 doubles per step but the first, for the largest steps[s]).  Vectors per slab: as many
// as the plan's 1 GB cap holds and as the transposed sampler's grid (one workgroup per 256 lanes and control node) allows, a multiple
// of 64; 0 where 64 vectors do not fit.  GEL_PROP_SLAB as in prop_slab().
static int64_t propadj_kmax(const gel_prop_plan* pl) {
  int64_t k = 1;
  for (const gel::PropPhaseDev& q : pl->ph) k = std::max<int64_t>(k, q.k);
  return k;
}
// Kg: the rows of the lane's wind column (16 Kg bytes), 0 where gwind is not wanted
static int64_t propadj_lane_bytes(const gel_prop_plan* pl, int64_t Kg = 0) {
  return 16 * pl->sampled_pts + 8 * (int64_t)pl->dev.S + 88 * (propadj_kmax(pl) - 1) + 16 * Kg;
}

static int64_t propadj_slab(const gel_prop_plan* pl, int64_t Q, int64_t Kg = 0) {
  const int64_t per_vec = 16 * pl->sampled_pts + Q * propadj_lane_bytes(pl, Kg);
  int64_t vs = std::min<int64_t>(kPropMaxSlab, kPropWsBytes / per_vec / 64 * 64);
  const int64_t grid_lanes = (int64_t)0x7fffffff / ((int64_t)pl->src->dims.N + 1) * gel::kPropAdjSampleThreads;
  vs = std::min<int64_t>(vs, std::min<int64_t>(grid_lanes, 0x7fffffff) / Q / 64 * 64);
  if (vs < 64) return 0;
  return slab_or_env(vs);
}

// every refusal that is decided before a buffer is looked at
static int propadj_refuse(const char* who, const gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, int64_t Kg = 0) {
  const std::string w(who);
  if (!plan) return fail(GEL_ERR_ARG, w + ": null plan");
  if (B < 0) return fail(GEL_ERR_ARG, w + ": B < 0");
  if (Q < 1) return fail(GEL_ERR_ARG, w + ": Q < 1");
  if ((int64_t)B * Q > 0x7fffffffLL) return fail(GEL_ERR_ARG, w + ": B Q exceeds 2^31 - 1 lanes");
  if (shared != 0 && shared != 1) return fail(GEL_ERR_ARG, w + ": shared is neither 0 nor 1");
  if (plan->flags & GEL_PROP_RESTART_NODE)
    return fail(GEL_ERR_ARG, w + ": a GEL_PROP_RESTART_NODE plan has no adjoint flight (neighbouring node segments share a stage point)");
  int64_t lane_steps = 0;   // a lane walks every phase, in section mode too (the inner checkpoints are the lane's)
  for (const gel::PropPhaseDev& q : plan->ph) lane_steps += (int64_t)q.k * q.n;
  if (lane_steps > gel::kPropMaxLaneSteps) return fail(GEL_ERR_ARG, w + ": the sum of steps[s] n_s exceeds 2^20 RK4 steps in one lane");
  if (!propadj_slab(plan, Q, Kg))
    return fail(GEL_ERR_ARG, w + ": the workspace of 64 vectors (control samples, and per functional the stage points' multipliers) exceeds the 1 GB cap");
  return GEL_OK;
}

static int propadj_check(const char* who, const gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const void* x, const void* lam,
                         const gel_wind_ensemble* ens, const void* y, const void* gx, const void* gwind = nullptr) {
  const std::string w(who);
  if (plan && !lam) return fail(GEL_ERR_ARG, w + ": lam is NULL");
  if (int rc = propadj_refuse(who, plan, B, Q, shared, (plan && gwind) ? prop_wind_rows(plan, ens) : 0)) return rc;
  if (int rc = ens_check(who, ens, plan->src, B)) return rc;
  if (plan->src->device == GEL_DEVICE_NONE) return fail(GEL_ERR_ARG, w + ": the plan's handle is host-only (GEL_DEVICE_NONE)");
  if (B > 0 && (!x || !y || !gx)) return fail(GEL_ERR_ARG, w + ": x, y or gx is NULL with B > 0");
  return GEL_OK;
}

int gel_prop_adjoint_info(const gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, int64_t* info) {
  if (!info) return fail(GEL_ERR_ARG, "gel_prop_adjoint_info: info is NULL");
  if (int rc = propadj_refuse("gel_prop_adjoint_info", plan, B, Q, shared)) return rc;
  const int64_t vs = propadj_slab(plan, Q);
  info[0] = propadj_lane_bytes(plan);
  info[1] = vs * Q;
  info[2] = (B + vs - 1) / vs;
  return GEL_OK;
}

// the launches of one call on stream s, slab after slab: the control samples and the value flight (y: the checkpoints; under an
// ensemble gel_propagate_ensemble*'s launch, so that the checkpoints are that flight's bits), the backward walk, the transposed
// sampler with the knot times
static int propadj_enqueue(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x, const double* d_disp,
                           const double* d_lam, const gel_wind_ensemble* ens, double* d_y, double* d_gx, double* d_gdisp, double* d_gwind,
                           hipStream_t s) {
  gel_problem* p = plan->src;
  const int64_t Kg = d_gwind ? prop_wind_rows(plan, ens) : 0;
  const int64_t vs = propadj_slab(plan, Q, Kg), ldv = std::min<int64_t>(vs, ((int64_t)B + 63) / 64 * 64);
  const int64_t gld = ldv * Q;
  const size_t set = 2 * (size_t)plan->sampled_pts;
  const size_t nck = 11 * (size_t)(propadj_kmax(plan) - 1);
  const size_t need = (size_t)ldv * set + (size_t)gld * (set + (size_t)plan->dev.S + nck + 2 * (size_t)Kg) + 1;   // (+ 1: ck is a valid pointer at k = 1 too)
  GROW_AFTER_DRAIN(p, plan->d_ws, need);
  double* const ws = plan->d_ws.get();
  double* const gws = ws + (size_t)ldv * set;    // the second region: the stage points' control multipliers
  double* const gS = gws + (size_t)gld * set;    // the third: the multiplier of S per (phase, lane)
  double* const ck = gS + (size_t)gld * (size_t)plan->dev.S;   // the fourth: the inner checkpoints of the interval in hand
  double* const gww = ck + (size_t)gld * nck + 1;              // the fifth: the lanes' wind columns [Kg][2][gld] (only where gwind is wanted)
  const auto [nv, ny, nd] = prop_strides(p);
  for (int64_t v0 = 0; v0 < B; v0 += vs) {
    const int nb = (int)std::min<int64_t>(vs, B - v0);
    const double* const disp = d_disp ? d_disp + (size_t)v0 * nd : nullptr;
    const gel::EnsDev e = ens_dev(ens, v0);   // the slab's part of the assignment, for the value flight and the walk alike
    HIPCHK(gel::launch_prop_slab(p->dev, plan->dev, plan->ph.data(), plan->n_max_sampled, nb, d_x + (size_t)v0 * nv, d_y + (size_t)v0 * ny, ws,
                                 ldv, disp, e, s));
    const size_t l0 = (size_t)v0 * Q;   // the slab's first lane
    gel::PropAdjArgs a{};
    a.nb = nb; a.Q = Q; a.shared = shared;
    a.x = d_x + (size_t)v0 * nv;
    a.disp = disp;
    a.lam = shared ? d_lam : d_lam + l0 * ny;
    a.y = d_y + (size_t)v0 * ny;
    a.gx = d_gx + l0 * nv;
    a.gdisp = d_gdisp ? d_gdisp + l0 * nd : nullptr;
    a.ws = ws; a.gws = gws; a.gS = gS; a.ck = ck; a.ld = ldv; a.gld = gld;
    gel::WindGradDev wg{};
    if (d_gwind) { wg.gww = gww; wg.gwind = d_gwind + l0 * 2 * (size_t)Kg; wg.Kg = (int32_t)Kg; }
    HIPCHK(gel::launch_propadj_slab(p->dev, plan->dev, a, e, wg, s));
  }
  return GEL_OK;
}

static int propadj_device(const char* who, gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x, const double* d_disp,
                          const double* d_lam, gel_wind_ensemble* ens, double* d_y, double* d_gx, double* d_gdisp, double* d_gwind = nullptr) {
  if (int rc = propadj_check(who, plan, B, Q, shared, d_x, d_lam, ens, d_y, d_gx, d_gwind)) return rc;
  if (B == 0) return GEL_OK;
  gel_problem* p = plan->src;
  HIPCHK(hipSetDevice(p->device));
  return propadj_enqueue(plan, B, Q, shared, d_x, d_disp, d_lam, ens, d_y, d_gx, d_gdisp, d_gwind, p->stream.get());
}

int gel_propagate_adjoint_ensemble_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x, const double* d_disp,
                                          const double* d_lam, gel_wind_ensemble* ens, double* d_y, double* d_gx, double* d_gdisp) {
  return propadj_device("gel_propagate_adjoint_ensemble_device", plan, B, Q, shared, d_x, d_disp, d_lam, ens, d_y, d_gx, d_gdisp);
}

int gel_propagate_adjoint_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x, const double* d_disp,
                                 const double* d_lam, double* d_y, double* d_gx, double* d_gdisp) {
  return propadj_device("gel_propagate_adjoint_device", plan, B, Q, shared, d_x, d_disp, d_lam, nullptr, d_y, d_gx, d_gdisp);
}

static int propadj_host(const char* who, gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp,
                        const double* lam, gel_wind_ensemble* ens, double* y, double* gx, double* gdisp, double* gwind = nullptr) {
  if (int rc = propadj_check(who, plan, B, Q, shared, x, lam, ens, y, gx, gwind)) return rc;
  if (B == 0) return GEL_OK;
  gel_problem* p = plan->src;
  HIPCHK(hipSetDevice(p->device));
  const auto [nv, ny, nd] = prop_strides(p);
  const size_t lanes = (size_t)B * Q;
  // (x, y, disp as gel_propagate_dispersed lays them out; the new buffers behind them)
  return staged_call(p, 0, {staged_in(x, (size_t)B * nv), staged_out(y, (size_t)B * ny), staged_in(disp, (size_t)B * nd),
                            staged_in(lam, (shared ? (size_t)Q : lanes) * ny), staged_out(gx, lanes * nv), staged_out(gdisp, lanes * nd),
                            staged_out(gwind, lanes * 2 * (size_t)prop_wind_rows(plan, ens))},
                     [&](const gel::ProblemDev&, double* const* a) {
                       return propadj_enqueue(plan, B, Q, shared, a[0], a[2], a[3], ens, a[1], a[4], a[5], a[6], p->stream.get());
                     });
}

int gel_propagate_adjoint_ensemble(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp,
                                   const double* lam, gel_wind_ensemble* ens, double* y, double* gx, double* gdisp) {
  return propadj_host("gel_propagate_adjoint_ensemble", plan, B, Q, shared, x, disp, lam, ens, y, gx, gdisp);
}

int gel_propagate_adjoint(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp, const double* lam,
                          double* y, double* gx, double* gdisp) {
  return propadj_host("gel_propagate_adjoint", plan, B, Q, shared, x, disp, lam, nullptr, y, gx, gdisp);
}

// the gradient with respect to the wind table's rows beside gx and gdisp; gwind == NULL: the calls above
int gel_propagate_adjoint_wind_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x, const double* d_disp,
                                      const double* d_lam, gel_wind_ensemble* ens, double* d_y, double* d_gx, double* d_gdisp, double* d_gwind) {
  return propadj_device("gel_propagate_adjoint_wind_device", plan, B, Q, shared, d_x, d_disp, d_lam, ens, d_y, d_gx, d_gdisp, d_gwind);
}

int gel_propagate_adjoint_wind(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp, const double* lam,
                               gel_wind_ensemble* ens, double* y, double* gx, double* gdisp, double* gwind) {
  return propadj_host("gel_propagate_adjoint_wind", plan, B, Q, shared, x, disp, lam, ens, y, gx, gdisp, gwind);
}

int gel_prop_adjoint_wind_info(const gel_prop_plan* plan, const gel_wind_ensemble* ens, int32_t B, int32_t Q, int32_t shared, int32_t want_gwind,
                               int64_t* info) {
  if (!info) return fail(GEL_ERR_ARG, "gel_prop_adjoint_wind_info: info is NULL");
  if (plan && ens && ens->src != plan->src) return fail(GEL_ERR_ARG, "gel_prop_adjoint_wind_info: the wind ensemble belongs to another handle");
  const int64_t Kg = plan ? prop_wind_rows(plan, ens) : 0, Kl = want_gwind ? Kg : 0;
  if (int rc = propadj_refuse("gel_prop_adjoint_wind_info", plan, B, Q, shared, Kl)) return rc;
  const int64_t vs = propadj_slab(plan, Q, Kl);
  info[0] = propadj_lane_bytes(plan, Kl);
  info[1] = vs * Q;
  info[2] = (B + vs - 1) / vs;
  info[3] = Kg;
  return GEL_OK;
}

}  // extern "C"
