// gel_host_mesh.hip -- the collocation error estimate per section (gel_mesh_*) and the batched spectral
// interpolation with its plan: dense output and mesh transfer (gel_interp*; 3.13).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gel_interp.h"
#include "gel_host_handle.h"

using namespace gelhost;

namespace {
constexpr const char* kNoGpuInterp = "host-only handle: the device interpolation needs a GPU (gel_interp_host runs on the host)";
}  // namespace

extern "C" {

// ------------- collocation error estimate per section -------------
#define MESH_FITS(p)                                                                                                   \
  do {                                                                                                                 \
    if (int rc_ = check_launch_lds("collocation error estimate", (p)->mesh.lds_max,                                    \
                                   gel::staged_table_doubles((p)->dev.Kw, (p)->dev.Kc),                                \
                                   gel::padded_table_doubles((p)->dev.Kw, (p)->dev.Kc), true))                         \
      return rc_;                                                                                                      \
  } while (0)
#define NEED_MESH(p)                                                                                                   \
  do {                                                                                                                 \
    if ((p)->mesh.hoff.empty())                                                                                        \
      return fail(GEL_ERR_ARG, "collocation error estimate: a phase has more than 511 nodes (one workgroup per point set)"); \
  } while (0)

int gel_mesh_dims(const gel_problem* p, int32_t* npts) {
  if (!p || !npts) return fail(GEL_ERR_ARG, "null argument");
  *npts = p->mesh.npts;
  return GEL_OK;
}

int gel_mesh_matrices(const gel_problem* p, int32_t phase, double* sigma, double* Lx, double* Lu, double* I) {
  if (!p || phase < 0 || phase >= p->dims.S) return fail(GEL_ERR_ARG, "bad argument");
  NEED_MESH(p);
  const int n = p->ph[phase].n, P = n + 1;
  const double* hb = p->mesh.host.data() + p->mesh.hoff[phase];
  if (sigma) std::memcpy(sigma, hb, (size_t)P * 8);
  if (Lx) std::memcpy(Lx, hb + P, (size_t)P * P * 8);
  if (Lu) std::memcpy(Lu, hb + P + (size_t)P * P, (size_t)P * n * 8);
  if (I) std::memcpy(I, hb + P + (size_t)P * P + (size_t)P * n, (size_t)P * P * 8);
  return GEL_OK;
}

int gel_mesh_error_device(gel_problem* p, int32_t B, const double* d_x, double* d_err, double* d_diff, void* stream) {
  if (!p || B < 1 || !d_x || !d_err) return fail(GEL_ERR_ARG, "bad argument");
  MESH_FITS(p);
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  NEED_MESH(p);
  HIPCHK(gel::launch_mesh(p->dev, p->mesh.dev, p->mesh.ph.data(), B, d_x, d_err, d_diff, stream_of(p, stream)));
  return GEL_OK;
}

int gel_mesh_error(gel_problem* p, int32_t B, const double* x, double* err, double* diff) {
  if (!p || B < 1 || !x || !err) return fail(GEL_ERR_ARG, "bad argument");
  MESH_FITS(p);
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  NEED_MESH(p);
  HIPCHK(hipSetDevice(p->device));
  return staged_call(p, kStagedZeroCopy,
                     {staged_in(x, (size_t)B * p->dims.num_vars), staged_out(err, (size_t)B * p->dims.S * 4), staged_out(diff, (size_t)B * p->mesh.npts * 11)},
                     [&](const gel::ProblemDev& dv, double* const* a) -> int {
                       HIPCHK(gel::launch_mesh(dv, p->mesh.dev, p->mesh.ph.data(), B, a[0], a[1], a[2], p->stream.get()));
                       return GEL_OK;
                     });
}

// ------------- batched spectral interpolation: dense output and mesh transfer -------------
// A plan = the matrices of every phase of the source handle at the plan's points, built here in extended precision from the
// handle's own tau with the barycentric machinery of the mesh estimate, rounded once; row-major on the host (gel_interp_matrices,
// gel_interp_host), transposed on the device (gel_interp.h).  It owns its tables and refers to the source handle for the device,
// the stream, the non-finite flag and the arena of the host-buffer form (staged_call): it is destroyed before that handle.
struct gel_interp_plan {
  gel_problem* src = nullptr;
  gel::InterpDev dev{};
  std::vector<gel::InterpPhaseDev> ph;
  std::vector<double> W;          // per phase Wx [P][n+1] | Wu [Pu][n], row-major, at woff[s]
  std::vector<size_t> woff;
  std::vector<double> pts;        // table mode: the points, phase after phase (ph[s].xd = the first of phase s)
  std::vector<int32_t> cp;        // copy_x | copy_u per phase (the device's array as it is)
  int64_t state_rows = 0;         // table: sum of the phases' points; transfer: the destination's M
  int n_max = 0;                  // longest source phase that has points
  DeviceArray<double> d_mat;
  DeviceArray<int32_t> d_cp;
  DeviceArray<gel::InterpPhaseDev> d_ph;
};

// Vectors per workgroup of an interpolation launch (what gel_interp_plan_info reports): the most whose staged slice fits, or
// GEL_INTERP_VB = 1 / 2 / 4 (measurement switch, read per call; a value whose slice does not fit is ignored).  The results do not
// depend on it.  0: not even one vector fits.
static int interp_vb(const gel_interp_plan* pl) {
  if (const char* e = getenv("GEL_INTERP_VB")) {
    const int w = atoi(e);
    if ((w == 1 || w == 2 || w == 4) && gel::interp_lds_bytes(pl->n_max, w) <= gel::kInterpMaxLds) return w;
  }
  return gel::interp_vectors_per_group(pl->n_max);
}

// points: per phase its state points zx [P] and control points zu [Pu] (fp64 numbers inside [-1, 1])
static int interp_plan_build(gel_problem* src, int mode, int32_t flags, const std::vector<std::vector<double>>& zx,
                             const std::vector<std::vector<double>>& zu, const std::vector<int32_t>& xd, const std::vector<int32_t>& ud,
                             int Md, int Nd, int64_t ostride, int64_t state_rows, gel_interp_plan** out) {
  const int S = src->dims.S;
  std::unique_ptr<gel_interp_plan> pl(new gel_interp_plan);
  pl->src = src;
  pl->state_rows = state_rows;
  pl->ph.resize(S);
  pl->woff.resize(S);
  std::vector<double> matT;   // the device's table: per phase WxT | WuT | sig
  for (int s = 0; s < S; s++) {
    const HostPhase& h = src->ph[s];
    const int n = h.n, P = (int)zx[s].size(), Pu = (int)zu[s].size();
    gel::InterpPhaseDev& q = pl->ph[s];
    q.n = n; q.xa = h.xa; q.ua = h.ua; q.P = P; q.Pu = Pu;
    q.ntile = (std::max(P, Pu) + gel::kInterpThreads - 1) / gel::kInterpThreads;
    q.xd = xd[s]; q.ud = ud[s];
    if (q.ntile) pl->n_max = std::max(pl->n_max, n);
    std::vector<ld> tx(n + 1), tc(n);
    tx[0] = -1.0L;
    for (int k = 0; k < n; k++) tx[k + 1] = tc[k] = (ld)h.tau[k];
    const std::vector<ld> wx = bary_weights(tx), wc = bary_weights(tc);
    pl->woff[s] = pl->W.size();
    q.cx = (int64_t)pl->cp.size();
    std::vector<ld> row(n + 1);
    for (int l = 0; l < P; l++) {
      lagrange_row(tx, wx, (ld)zx[s][l], row.data());
      int32_t c = -1;
      for (int i = 0; i <= n; i++) {
        pl->W.push_back((double)row[i]);
        if ((double)tx[i] == zx[s][l]) c = i;
      }
      pl->cp.push_back(c);
    }
    q.cu = (int64_t)pl->cp.size();
    for (int l = 0; l < Pu; l++) {
      lagrange_row(tc, wc, (ld)zu[s][l], row.data());
      int32_t c = -1;
      for (int j = 0; j < n; j++) {
        pl->W.push_back((double)row[j]);
        if ((double)tc[j] == zu[s][l]) c = j;
      }
      pl->cp.push_back(c);
    }
    const double* Wx = pl->W.data() + pl->woff[s];
    const double* Wu = Wx + (size_t)P * (n + 1);
    q.wx = (int64_t)matT.size();
    for (int i = 0; i <= n; i++)
      for (int l = 0; l < P; l++) matT.push_back(Wx[(size_t)l * (n + 1) + i]);
    q.wu = (int64_t)matT.size();
    for (int j = 0; j < n; j++)
      for (int l = 0; l < Pu; l++) matT.push_back(Wu[(size_t)l * n + j]);
    q.sg = (int64_t)matT.size();
    if (mode == 0) {
      matT.insert(matT.end(), zx[s].begin(), zx[s].end());
      pl->pts.insert(pl->pts.end(), zx[s].begin(), zx[s].end());
    }
  }
  gel::InterpDev& d = pl->dev;
  d.S = S; d.mode = mode; d.unit_quat = (flags & GEL_INTERP_UNIT_QUAT) ? 1 : 0;
  d.nvars = src->dims.num_vars; d.M = src->dims.M; d.N = src->dims.N;
  d.Md = Md; d.Nd = Nd; d.ostride = ostride;
  if (src->device != GEL_DEVICE_NONE) {
    if (pl->n_max && !gel::interp_vectors_per_group(pl->n_max))
      return fail(GEL_ERR_ARG, "interpolation plan: a phase's staged slice (13 n + 11 doubles) does not fit a workgroup's LDS "
                               "(gel_interp_host on a host-only handle has no such limit)");
    HIPCHK(hipSetDevice(src->device));
    HIPCHK(pl->d_mat.upload(matT));
    HIPCHK(pl->d_cp.upload(pl->cp));
    HIPCHK(pl->d_ph.upload(pl->ph));
    d.ph = pl->d_ph.get(); d.mat = pl->d_mat.get(); d.cp = pl->d_cp.get();
  }
  *out = pl.release();
  return GEL_OK;
}

int gel_interp_plan_create(gel_problem* src, const int32_t* npts, const double* pts, int32_t flags, gel_interp_plan** out) {
  if (!src || !npts || !out || (flags & ~GEL_INTERP_UNIT_QUAT)) return fail(GEL_ERR_ARG, "bad argument");
  const int S = src->dims.S;
  int64_t total = 0;
  for (int s = 0; s < S; s++) {
    if (npts[s] < 0) return fail(GEL_ERR_ARG, "interpolation plan: negative npts");
    total += npts[s];
  }
  if (total > 0 && !pts) return fail(GEL_ERR_ARG, "null argument");
  if (total * gel::kInterpCols > 0x7fffffffLL) return fail(GEL_ERR_ARG, "interpolation plan: too many points");
  for (int64_t k = 0; k < total; k++)
    if (!(pts[k] >= -1.0 && pts[k] <= 1.0)) return fail(GEL_ERR_ARG, "interpolation plan: a point is not a finite number inside [-1, 1]");
  std::vector<std::vector<double>> z(S);
  std::vector<int32_t> xd(S), ud(S, 0);
  int64_t o = 0;
  for (int s = 0; s < S; s++) {
    z[s].assign(pts + o, pts + o + npts[s]);
    xd[s] = (int32_t)o;
    o += npts[s];
  }
  return interp_plan_build(src, 0, flags, z, z, xd, ud, 0, 0, total * gel::kInterpCols, total, out);
}

int gel_interp_plan_create_transfer(gel_problem* src, const gel_problem* dst, int32_t flags, gel_interp_plan** out) {
  if (!src || !dst || !out || (flags & ~GEL_INTERP_UNIT_QUAT)) return fail(GEL_ERR_ARG, "bad argument");
  if (src->dims.S != dst->dims.S) return fail(GEL_ERR_ARG, "mesh transfer: the two handles differ in their number of phases");
  const int S = src->dims.S;
  std::vector<std::vector<double>> zx(S), zu(S);
  std::vector<int32_t> xd(S), ud(S);
  for (int s = 0; s < S; s++) {
    const HostPhase& h = dst->ph[s];
    zu[s] = h.tau;
    zx[s].push_back(-1.0);
    zx[s].insert(zx[s].end(), h.tau.begin(), h.tau.end());
    for (double v : h.tau)
      if (!(v >= -1.0 && v <= 1.0)) return fail(GEL_ERR_ARG, "mesh transfer: a destination node lies outside [-1, 1]");
    xd[s] = h.xa; ud[s] = h.ua;
  }
  return interp_plan_build(src, 1, flags, zx, zu, xd, ud, dst->dims.M, dst->dims.N, dst->dims.num_vars, dst->dims.M, out);
}

int gel_interp_plan_destroy(gel_interp_plan* plan) {
  if (!plan) return GEL_OK;
  if (plan->src->device != GEL_DEVICE_NONE) {
    hipSetDevice(plan->src->device);
    (void)drain(plan->src);   // a resident call in flight still reads the plan's tables
  }
  delete plan;
  return GEL_OK;
}

int gel_interp_plan_info(const gel_interp_plan* plan, int64_t* info) {
  if (!plan || !info) return fail(GEL_ERR_ARG, "null argument");
  info[0] = plan->dev.S; info[1] = plan->dev.mode; info[2] = plan->state_rows; info[3] = plan->dev.ostride;
  info[4] = plan->dev.nvars; info[5] = interp_vb(plan);
  return GEL_OK;
}

int gel_interp_matrices(const gel_interp_plan* plan, int32_t phase, double* Wx, double* Wu, int32_t* copy_x, int32_t* copy_u) {
  if (!plan || phase < 0 || phase >= plan->dev.S) return fail(GEL_ERR_ARG, "bad argument");
  const gel::InterpPhaseDev& q = plan->ph[phase];
  const double* w = plan->W.data() + plan->woff[phase];
  if (Wx) std::memcpy(Wx, w, (size_t)q.P * (q.n + 1) * 8);
  if (Wu) std::memcpy(Wu, w + (size_t)q.P * (q.n + 1), (size_t)q.Pu * q.n * 8);
  if (copy_x) std::memcpy(copy_x, plan->cp.data() + q.cx, (size_t)q.P * 4);
  if (copy_u) std::memcpy(copy_u, plan->cp.data() + q.cu, (size_t)q.Pu * 4);
  return GEL_OK;
}

int gel_interp_host(const gel_interp_plan* plan, int32_t B, const double* x, double* out) {
  if (!plan || B < 0 || (B > 0 && (!x || !out))) return fail(GEL_ERR_ARG, "bad argument");
  const gel::InterpDev& d = plan->dev;
  const int M = d.M, N = d.N, Md = d.Md;
  bool bad = false;
  auto put = [&bad](double* o, double v) { *o = v; bad |= !std::isfinite(v); };
  for (int32_t b = 0; b < B; b++) {
    const double* xb = x + (size_t)b * d.nvars;
    double* ob = out + (size_t)b * d.ostride;
    const double* tk = xb + 11 * M + 2 * N;
    for (int s = 0; s < d.S; s++) {
      const gel::InterpPhaseDev& q = plan->ph[s];
      const int n = q.n;
      const double* Wx = plan->W.data() + plan->woff[s];
      const double* Wu = Wx + (size_t)q.P * (n + 1);
      const int32_t* cx = plan->cp.data() + q.cx;
      const int32_t* cu = plan->cp.data() + q.cu;
      // component c of state row xa + i
      auto X = [&](int i, int c) {
        const int xi = q.xa + i;
        return (c == 0) ? xb[xi] : (c < 4) ? xb[M + 3 * xi + (c - 1)] : (c < 7) ? xb[4 * M + 3 * xi + (c - 4)] : xb[7 * M + 4 * xi + (c - 7)];
      };
      for (int l = 0; l < q.P; l++) {
        double a[11];
        if (cx[l] >= 0) {
          for (int c = 0; c < 11; c++) a[c] = X(cx[l], c);
        } else {
          for (int c = 0; c < 11; c++) {
            double acc = 0.0;
            for (int i = 0; i <= n; i++) acc = __builtin_fma(Wx[(size_t)l * (n + 1) + i], X(i, c), acc);
            a[c] = acc;
          }
          if (d.unit_quat) {
            const double qv[4] = {a[7], a[8], a[9], a[10]};
            const double nrm = std::sqrt(gel::interp_quat_dot(qv));
            for (int k = 0; k < 4; k++) a[7 + k] = qv[k] / nrm;
          }
        }
        if (d.mode == 0) {
          double* o = ob + (size_t)(q.xd + l) * gel::kInterpCols;
          put(o, gel::interp_time(plan->pts[(size_t)q.xd + l], tk[s], tk[s + 1]));
          for (int c = 0; c < 11; c++) put(o + 1 + c, a[c]);
        } else {
          const int xi = q.xd + l;
          put(ob + xi, a[0]);
          for (int c = 0; c < 3; c++) put(ob + Md + 3 * xi + c, a[1 + c]);
          for (int c = 0; c < 3; c++) put(ob + 4 * Md + 3 * xi + c, a[4 + c]);
          for (int c = 0; c < 4; c++) put(ob + 7 * Md + 4 * xi + c, a[7 + c]);
        }
      }
      for (int l = 0; l < q.Pu; l++) {
        double u[2];
        for (int c = 0; c < 2; c++) {
          if (cu[l] >= 0) { u[c] = xb[11 * M + 2 * (q.ua + cu[l]) + c]; continue; }
          double acc = 0.0;
          for (int j = 0; j < n; j++) acc = __builtin_fma(Wu[(size_t)l * n + j], xb[11 * M + 2 * (q.ua + j) + c], acc);
          u[c] = acc;
        }
        double* o = (d.mode == 0) ? ob + (size_t)(q.xd + l) * gel::kInterpCols + 12 : ob + 11 * Md + 2 * (q.ud + l);
        put(o, u[0]);
        put(o + 1, u[1]);
      }
    }
    if (d.mode == 1)
      for (int s = 0; s <= d.S; s++) put(ob + 11 * Md + 2 * d.Nd + s, tk[s]);
  }
  return bad ? GEL_NONFINITE : GEL_OK;
}

int gel_interp_resident(gel_interp_plan* plan, int32_t B, const double* d_x, double* d_out) {
  if (!plan || B < 0 || (B > 0 && (!d_x || !d_out))) return fail(GEL_ERR_ARG, "bad argument");
  gel_problem* p = plan->src;
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuInterp);
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(gel::launch_interp(plan->dev, plan->ph.data(), plan->n_max, B, d_x, d_out, p->d_flag.get(), interp_vb(plan), p->stream.get()));
  return GEL_OK;
}

int gel_interp(gel_interp_plan* plan, int32_t B, const double* x, double* out) {
  if (!plan || B < 0 || (B > 0 && (!x || !out))) return fail(GEL_ERR_ARG, "bad argument");
  gel_problem* p = plan->src;
  NEED_DEVICE(p, GEL_ERR_ARG, kNoGpuInterp);
  if (B == 0 || plan->dev.ostride == 0) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  return staged_call(p, 0, {staged_in(x, (size_t)B * plan->dev.nvars), staged_out(out, (size_t)B * plan->dev.ostride)},
                     [&](const gel::ProblemDev&, double* const* a) -> int {
                       HIPCHK(gel::launch_interp(plan->dev, plan->ph.data(), plan->n_max, B, a[0], a[1], p->d_flag.get(), interp_vb(plan),
                                                 p->stream.get()));
                       return GEL_OK;
                     });
}

}  // extern "C"
