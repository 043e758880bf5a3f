// gel_aero_body.h -- the aero path constraints' rows as a device function of a (virtual) workgroup index: AeroOut, the park of a
// wavefront and aero_body, which the three aero kernels (gel_kernels_aerorows.hip) and callback_kernel (gel_kernels.hip) run.
#pragma once
#include "gel_tables.h"

namespace gel {

// Aero path constraints: lib/con_aero.py:90-252 (values) and :311-756 (forward-
// difference gradients), device functions of src/wrapper_utils.hpp:89-206.  kind 0 = angle of attack,
// 1 = dynamic pressure, 2 = q*alpha.
//
// ONE launch serves all three kinds.  A constrained state node (phase, k) appears once, whatever kinds constrain it,
// and the chain (geodetic -> wind -> Earth angle -> wind in ECI -> air-relative velocity; thrust direction / atmosphere)
// is split by what each piece depends on, as in gel_rhs_parts.h: a sweep recomputes only what its perturbed variable
// enters (a reused piece is bit-identical to what the reference's full re-evaluation produces, because the perturbed
// variable does not enter it).  Eight lanes per node: lane 0 the centre value plus the light sweeps (velocity 3:
// only the air-relative velocity changes; quaternion 4: only the thrust direction), lanes 1..3 one position sweep
// each (the whole chain), lanes 4..5 the t0 / tf sweeps (Earth angle -> wind rotation -> air-relative velocity).  The
// centre values reach the other lanes by a wavefront shuffle.  4 + 2 heavy evaluations per node instead of the
// 3 kinds x 13 of one-lane-per-row.
// ---------------------------------------------------------------------------
struct AeroOut {
  double* con[3];   // [B][nrows[kind]]
  double* jac[3];   // [B][nrows[kind] * (8 + 4 (kind != 1))]: position | velocity | quaternion | t blocks
  int32_t nrows[3];
  int64_t ld;       // != 0: the outputs are per-vector RECORDS of ld doubles (gel_eval_batch_aero_device): con / jac point at the
                    // kind's part of record 0, a vector's part lies b * ld doubles on; 0: dense [B][...] arrays per kind
  int32_t sm;       // != 0 (records only): SPEC-MAJOR part A (gel_device.h AeroPhaseDev) -- a node's row0[kind] is the first double of
                    // its spec's block in the record, row[kind] its constraint value's place; con / jac all point at the record
};

// One WAVEFRONT = 64 consecutive constrained nodes of one decision vector, every sweep of the node in the same lane (round 2 ran
// one wavefront per sweep role and the whole chain in each: six, then four runs of the atmosphere chain per node):
//   centre      pos_part<CENTRE> (the fused kernel's position part without gravity), wind into ECI, air-relative velocity
//               (the rotation by omega t and back is not performed: gel_rhs_parts.h aero_force), alpha, q;
//   position    EXACT-DIFFERENCE form (pos_delta(), gel_rhs_parts.h): the change of latitude pair, altitude, density and wind
//               from algebraic identities of the reference's formulas, ~130 operations instead of a second run of the chain,
//               then wind -> air velocity -> alpha, q at the perturbed point; a wavefront with a lane the form does not
//               cover (another atmosphere layer / table piece, next to the polar axis) recomputes that sweep in full;
//   velocity    only the air-relative velocity changes;   quaternion: only the body axis;
//   t0 / tf     zeros: their sweeps (con_aero.py:452-463 and twins) move only the Earth angle, which the air-relative velocity
//               does not depend on -- the rotation is applied and undone, and the NED axes at an inertial position do not move
//               with t -- so the reference's quotients are rounding noise around zero (<= 9e-5 beside position entries of 3e3).
// GEL_FLAG_FD_RECOMPUTE: every position sweep and the two t sweeps re-run the chain like the reference.  alpha is only
// evaluated by wavefronts that have an alpha or q-alpha row.  Consecutive lanes are consecutive nodes of a spec, so every
// store of a gradient block is one contiguous segment (which is what lets the B = 1 callback write straight into pinned
// host memory).  Four wavefronts (four tiles) per workgroup.
constexpr int kAeroWaves = 4;
// aero_vair2(), aero_cos(), aero_acos(), aero_dalpha(): gel_rhs_parts.h (shared with the fused kernel's aero rows)
// park slots of one wavefront (doubles; the last six hold up to 12 ints per lane)
enum { AP_ILIM = 0, AP_AC = 3, AP_QC, AP_CC, AP_IS, AP_IND, AP_W = 8, AP_A0 = 11, AP_DIR = 14, AP_RHO = 17, AP_NV2 = 18, AP_INTS = 19,
       kAeroParkSlots = 25 };
typedef __attribute__((address_space(3))) int lds_int;
typedef __attribute__((address_space(3))) double lds_f64;
// ROLES (the B = 1 callback launch, where the length of one wavefront's chain is what counts): the four wavefronts of a
// workgroup share ONE tile -- wavefront 0 the centre values and the light sweeps, wavefronts 1..3 the centre and one position
// sweep each.  Same operations on the same operands per entry: bit-identical to the one-wavefront form.
// WIDE (the rows the fused kernel's lanes do not reach -- state node 0 of every phase, phases without aerodynamics -- of a launch
// whose outputs are the per-vector records of gel_eval_batch_aero_device): any number of vectors per wavefront (entry f of the
// (vector, node) sequence -> vector f / nnodes), outputs at 64-bit addresses b * ld + ... by plain global stores.  Same
// expressions per entry, same bits.
// SM (records only): SPEC-MAJOR part A (AeroOut::sm) -- an instantiation of its own, so that the ordinary launches carry neither
// its selects nor a third form of every store (as a run-time switch it cost aero_kernel 8 %)
template <bool ROLES, bool WIDE = false, bool SM = false>
__device__ __forceinline__ void aero_body(const ProblemDev P, int nnodes, const AeroNodeDev* __restrict__ nodes, int tiles, int B,
                                          const double* __restrict__ x, const AeroOut O, const unsigned vblk) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds);
  const int lane = (int)(threadIdx.x & 63);
  const int sw = ROLES ? (int)(threadIdx.x >> 6) : -1;   // ROLES: 0 centre + light sweeps, 1..3 position sweep sw - 1
  const long long wid = ROLES ? (long long)vblk : (long long)vblk * kAeroWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // FLAT (batch launches, tiles == 0) [r5]: a wavefront takes 64 consecutive entries of the (vector, node) sequence of the whole batch,
  // whichever vectors they belong to -- 325 constrained nodes per vector are 5.08 wavefronts' worth, not six tiles with the last one
  // 59 / 64 empty.  A wavefront then straddles at most two vectors (nnodes >= 64), so the vector is a per-lane value.
  const bool flat = !ROLES && !WIDE && tiles == 0;
  int b, ni_raw;
  bool live;
  if (WIDE) {
    const long long total = (long long)B * nnodes, f = wid * 64 + lane;
    if (wid * 64 >= total) return;                      // after the tables' barrier
    live = f < total;
    const long long fc = live ? f : total - 1;
    b = (int)(fc / nnodes);
    ni_raw = live ? (int)(fc - (long long)b * nnodes) : nnodes;
  } else if (flat) {
    const long long total = (long long)B * nnodes, f0 = wid * 64;
    if (f0 >= total) return;                           // after the tables' barrier
    const int b0 = (int)(f0 / nnodes), r0 = (int)(f0 - (long long)b0 * nnodes);
    const bool wrap = r0 + lane >= nnodes;
    live = f0 + lane < total;
    b = live ? (wrap ? b0 + 1 : b0) : b0;
    ni_raw = live ? (wrap ? r0 + lane - nnodes : r0 + lane) : nnodes;
  } else {
    if (wid >= (long long)B * tiles) return;           // after the tables' barrier
    b = (int)(wid / tiles);
    ni_raw = (int)(wid - (long long)b * tiles) * 64 + lane;
    live = ni_raw < nnodes;
  }
  const int ni = live ? ni_raw : nnodes - 1;
  const AeroNodeDev Nd = nodes[ni];
  const PhaseDev& ph = P.phases[Nd.phase];
  const double* xb = x + (size_t)b * P.nvars;
  const int M = P.M, N = P.N, xi = ph.xa + Nd.k;
  const double dx = P.dx;
  double re[3];
#pragma unroll
  for (int c = 0; c < 3; c++) re[c] = xb[M + 3 * xi + c];
  const bool want_jac = O.jac[0] || O.jac[1] || O.jac[2];
  // does any lane of this wavefront have an alpha or q-alpha row?  (wave-uniform)
  const bool need_alpha = __builtin_amdgcn_ballot_w64(live && ((O.con[0] && Nd.row[0] >= 0) || (O.con[2] && Nd.row[2] >= 0))) != 0;
  // The park: this wavefront's [slot][lane] region of LDS behind the tables.  What every store needs (1/limit, the centre's alpha,
  // q, cos, 1/sin, the node's rows) and what only the light sweeps need (centre wind, air velocity, body axis) wait there
  // instead of in registers across the position sweeps (234 -> 164 VGPRs).
  lds_f64* park = (lds_f64*)lds + ((table_doubles(P.Kw, P.Kc) + 1) & ~1) + (size_t)(threadIdx.x >> 6) * (kAeroParkSlots * 64) + lane;
  // ints (12 per lane): [kind] 8 nk; then per kind and block width w the BYTE offset 8 (w row0 + k) of this node's entries inside a
  // block of that width (or -1: no row of this kind / no gradient asked) -- alpha: w = 3, 4, 2 at 3, 4, 5; q: w = 3, 2 at 6, 7;
  // q-alpha: w = 3, 4, 2 at 8, 9, 10; [11] centre_ok.  An entry of block (bo, w), column col then sits at byte
  // 8 bo R + col (8 nk) + that offset of the kind's gradient vector: one 32-bit multiply-add per store, the rest on the scalar unit
  // (round 4 formed bo R + w row0 + col nk + k in 64-bit vector arithmetic per entry and kind: 369 of the 2,349 vector instructions
  // of a tile were integer address work)
  lds_int* ipark = (lds_int*)(park - lane + AP_INTS * 64) + lane;
#define AP_AIDX(kind, w) ((kind) == 0 ? ((w) == 3 ? 3 : ((w) == 4 ? 4 : 5)) : ((kind) == 1 ? ((w) == 3 ? 6 : 7) : ((w) == 3 ? 8 : ((w) == 4 ? 9 : 10))))
#define AP_GET(i) (park[(i) * 64])
#define AP_SET(i, v) (park[(i) * 64] = (v))
  // ---- centre (con_aero.py:39-87: scale, evaluate)
  PosCentre pc;
  PosPart pp;
  EarthAngle ea{1.0, 0.0, 1.0, 0.0};
  // Calm air [r5]: where both wind components of every lane are exactly zero (below and above the measured part of the wind table: in
  // the shipped example below 1 km and from 23 km up) the rotation of the zero vector into ECI is the zero vector -- wind_eci_or_calm()
  // skips its ~70 instructions, four times per tile -- and the Earth angle, which enters the air-relative velocity only through that
  // rotation (aero_vair2), is not formed at all (as in the fused kernel).  Nor is it where the air moves: wind_eci() reads the angle
  // only in a lane exactly on the polar axis, so the vote is wind_needs_angle() -- windy AND on the axis -- at the centre and, from
  // the node's time read again, in any sweep whose perturbed point is the first to need it.
  bool have_ea = false;
#define GEL_AERO_NEED_EA(ip_, wn_, we_)                                                                                \
  do {                                                                                                                 \
    if (!have_ea && __builtin_amdgcn_ballot_w64(wind_needs_angle(ip_, wn_, we_)) != 0) {                                \
      const int kn_ = nodes[ni].k, phn_ = nodes[ni].phase;                                                             \
      const double to_ = xb[11 * M + 2 * N + phn_], tf_ = xb[11 * M + 2 * N + phn_ + 1];                               \
      const double tau_ = (kn_ == 0) ? 0.0 : P.tau[P.phases[phn_].toff + kn_ - 1];                                     \
      /* PSparams.time_nodes (SectionParameters.py:77-81): node 0 is t0 itself; t in seconds here (con_aero.py:45) */   \
      ea = earth_angle(((kn_ == 0) ? to_ : (tau_ * (tf_ - to_) / 2 + (tf_ + to_) / 2)) * P.ut);                         \
      have_ea = true;                                                                                                  \
    }                                                                                                                  \
  } while (0)
  double chk = 0.0;
  {
    double r[3], v[3], q[4], w[3], a0[3], dir[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { r[c] = re[c] * P.up; v[c] = xb[4 * M + 3 * xi + c] * P.uv; }
#pragma unroll
    for (int c = 0; c < 4; c++) q[c] = xb[7 * M + 4 * xi + c];
    PosCentreTail pt;
    pp = pos_part<true, PosCentreSink, false>(r, tb, 0.0, nullptr, PosCentreSink{&pc}, &pt);
    pos_centre_tail(pt, pp.rho, pp.P, tb, pc, pp.wn, pp.we);
    GEL_AERO_NEED_EA(pp.inv_p, pp.wn, pp.we);
    wind_eci_or_calm(r, ea, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, w);
    const double nv2 = aero_vair2(r, v, w, a0);
    thrust_dir(q, dir);
    const double ind = frsqrt(fmax(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2], 1.0e-300));
    const double cc = need_alpha ? aero_cos(a0, nv2, dir, ind) : 0.0;
    const double alpha_c = need_alpha ? aero_acos(cc, nv2) : 0.0;
    const double qdyn_c = 0.5 * pp.rho * nv2;                       // 0.5 rho |v_air|^2 (wrapper_utils.hpp:163-175)
    double sc, isc;
    fsqrt_rsqrt(fmax((1.0 - cc) * (1.0 + cc), 1.0e-300), sc, isc);  // sin(alpha_c) and its reciprocal
    const bool centre_ok = (cc <= 1.0) && (nv2 >= 1.0e-12) && (sc > 1.0e-6);
    // f / units[3] (con_aero.py:85-87) as f * (1 / units[3]) (one rounding apart from the division); con = 1 - f (:127-139)
#pragma unroll
    for (int kind = 0; kind < 3; kind++) {
      const double il = frcp(Nd.limit[kind]);
      AP_SET(AP_ILIM + kind, il * P.inv_dx);   // 1 / (limit dx): what every gradient entry of the kind is scaled by
      const int row = Nd.row[kind];
      {
        const bool has = live && O.jac[kind] && row >= 0;
        // FLAT: the vector's gradient values start b R (8 + nq) doubles into the kind's buffer (unsigned 32-bit byte offsets: the
        // launcher keeps to the per-vector mapping where a batch's gradients exceed 4 GB); -1 = no entry
        const unsigned vb = flat ? (unsigned)b * (unsigned)(O.ld ? (int)O.ld * 8 : O.nrows[kind] * (8 + ((kind == 1) ? 0 : 4)) * 8) : 0u;
        ipark[kind * 64] = 8 * Nd.nk[kind];
        ipark[AP_AIDX(kind, 3) * 64] = has ? (int)(vb + 8u * (unsigned)((SM ? 1 : 3) * Nd.row0[kind] + Nd.ko)) : -1;
        ipark[AP_AIDX(kind, 2) * 64] = has ? (int)(vb + 8u * (unsigned)((SM ? 1 : 2) * Nd.row0[kind] + Nd.ko)) : -1;
        if (kind != 1) ipark[AP_AIDX(kind, 4) * 64] = has ? (int)(vb + 8u * (unsigned)((SM ? 1 : 4) * Nd.row0[kind] + Nd.ko)) : -1;
      }
      if (!live || row < 0 || !O.con[kind] || (ROLES && sw != 0)) continue;
      const double cv = 1.0 - ((kind == 0) ? alpha_c : (kind == 1) ? qdyn_c : qdyn_c * alpha_c) * il;
      if (ROLES) __builtin_nontemporal_store(cv, O.con[kind] + (size_t)b * O.nrows[kind] + row);
      else if (WIDE) O.con[kind][(size_t)b * O.ld + row] = cv;
      else O.con[kind][(size_t)b * (O.ld ? (size_t)O.ld : (size_t)O.nrows[kind]) + row] = cv;
      chk += cv;
    }
    ipark[11 * 64] = centre_ok ? 1 : 0;
    AP_SET(AP_AC, alpha_c); AP_SET(AP_QC, qdyn_c); AP_SET(AP_CC, cc); AP_SET(AP_IS, isc); AP_SET(AP_IND, ind);
#pragma unroll
    for (int c = 0; c < 3; c++) { AP_SET(AP_W + c, w[c]); AP_SET(AP_A0 + c, a0[c]); AP_SET(AP_DIR + c, dir[c]); }
    AP_SET(AP_RHO, pp.rho); AP_SET(AP_NV2, nv2);
  }
  // One gradient entry of every kind that has this node, jac = -(f_p - f_c)/dx (con_aero.py:437-463), from the perturbed point's
  // air velocity a (squared norm nv2), body axis d (1/|d| = ind) and density: alpha_p - alpha_c in exact-difference form
  // (aero_dalpha; a lane it does not cover takes two acos like the reference -- per lane, so that a node's values do not depend on
  // which nodes share its wavefront: the flat mapping puts two vectors' nodes into one), q_p - q_c as it is, and
  //   alpha:   d f = t / limit        q:   d f = (q_p - q_c) / limit        q alpha:   d f = (q_p t + (q_p - q_c) alpha_c) / limit
  // (q_p alpha_p - q_c alpha_c, regrouped).  Block offset `boff` in units of R rows (0 position, 3 velocity, 6 quaternion, -1 = t:
  // 6 + nq), `width` columns per row, column `col`; zero: the entry is an exact zero.
#define GEL_AERO_EMIT(boff, width, col, a, nv2, d, ind, rho, skip_q, zero, skip_lane)                                      \
  do {                                                                                                            \
    double t_ = 0.0, dq_ = 0.0, qp_ = 0.0;                                                                        \
    const double ac_ = AP_GET(AP_AC);                                                                             \
    if (!(zero)) {                                                                                                \
      const double qc_ = AP_GET(AP_QC);                                                                           \
      qp_ = 0.5 * (rho) * (nv2);                                                                                  \
      dq_ = qp_ - qc_;                                                                                            \
      if (need_alpha) {                                                                                           \
        const double cp_ = aero_cos(a, nv2, d, ind);                                                              \
        const bool okd_ = aero_dalpha(cp_, nv2, AP_GET(AP_CC), AP_GET(AP_IS), ipark[11 * 64] != 0, t_);           \
        if (__builtin_amdgcn_ballot_w64(!okd_) != 0) {                                                            \
          const double t2_ = aero_acos(cp_, nv2) - ac_;                                                           \
          t_ = okd_ ? t_ : t2_;                                                                                   \
        }                                                                                                         \
      }                                                                                                           \
    }                                                                                                             \
    _Pragma("unroll") for (int kind = 0; kind < 3; kind++) {                                                      \
      if ((skip_q) && kind == 1) continue;                 /* dynamic pressure has no quaternion block */        \
      const int a8_ = ipark[AP_AIDX(kind, width) * 64];                                                           \
      if (a8_ == -1 || (skip_lane)) continue;                                                                     \
      if (SM && (zero)) continue;                          /* spec-major records do not hold the exact zeros of the t columns */ \
      const int nq = (kind == 1) ? 0 : 4;                                                                         \
      const int bo = ((boff) < 0) ? (6 + nq) : (boff);                                                            \
      const double df_ = (kind == 0) ? t_ : ((kind == 1) ? dq_ : qp_ * t_ + dq_ * ac_);                           \
      const double gv = (zero) ? 0.0 : -(df_ * AP_GET(AP_ILIM + kind));                                           \
      gel_au2 gd_;                                                                                                \
      __builtin_memcpy(&gd_, &gv, 8);                                                                             \
      if (WIDE) O.jac[kind][(size_t)b * O.ld + (size_t)bo * O.nrows[kind] + ((a8_ + (col) * ipark[kind * 64]) >> 3)] = gv;                     \
      else if (SM) __builtin_amdgcn_raw_buffer_store_b64(gd_, jrs[kind], a8_ + ((((boff) < 0) ? 11 : ((boff) == 0 ? 1 : ((boff) == 3 ? 4 : 7))) + (col)) * ipark[kind * 64], 0, 0); \
      else __builtin_amdgcn_raw_buffer_store_b64(gd_, jrs[kind], ((col) == 0) ? a8_ : a8_ + (col) * ipark[kind * 64], 8 * bo * O.nrows[kind], ROLES ? 2 : 0); /* ROLES = the one-vector callback: streamed to pinned host memory */ \
      chk += gv;                                                                                                  \
    }                                                                                                             \
  } while (0)
  // one buffer resource per kind: base = this vector's gradient values, [R][8 + nq] doubles (wave-uniform: scalar registers)
  typedef unsigned gel_au2 __attribute__((ext_vector_type(2)));
  __amdgpu_buffer_rsrc_t jrs[3];
#pragma unroll
  for (int kind = 0; kind < 3; kind++)
    jrs[kind] = __builtin_amdgcn_make_buffer_rsrc((O.jac[kind] && !WIDE) ? (void*)(O.jac[kind] + (flat ? (size_t)0 : (size_t)__builtin_amdgcn_readfirstlane(b) * (O.ld ? (size_t)O.ld : (size_t)O.nrows[kind] * (8 + ((kind == 1) ? 0 : 4))))) : (void*)nullptr,
                                                  0, -1, 0x00020000);
  if (want_jac) {
    // ---- t0 / tf columns
#pragma unroll 1
    for (int c = (ROLES && sw != 0) ? 2 : 0; c < 2; c++) {
      if (P.fd_recompute) {   // audit form: the knot times and the node's abscissa are read again (not carried in registers)
        const int kn = nodes[ni].k, phn = nodes[ni].phase;
        const double to2 = xb[11 * M + 2 * N + phn], tf2 = xb[11 * M + 2 * N + phn + 1];
        const double tau2 = (kn == 0) ? 0.0 : P.tau[P.phases[phn].toff + kn - 1];
        const double to_p = (c == 0) ? to2 + dx : to2, tf_p = (c == 1) ? tf2 + dx : tf2;
        const double tp = ((kn == 0) ? to_p : (tau2 * (tf_p - to_p) / 2 + (tf_p + to_p) / 2)) * P.ut;
        const EarthAngle eq = earth_angle(tp);
        const double r[3] = {fresh_product(re[0], P.up), fresh_product(re[1], P.up), fresh_product(re[2], P.up)};
        const double vq[3] = {xb[4 * M + 3 * xi] * P.uv, xb[4 * M + 3 * xi + 1] * P.uv, xb[4 * M + 3 * xi + 2] * P.uv};
        double wq[3], aq[3];
        wind_eci_chain(r, eq, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, wq);   // the reference's chain: see wind_eci_chain_or_calm()
        const double nvq = aero_vair2(r, vq, wq, aq);
        const double dq[3] = {AP_GET(AP_DIR), AP_GET(AP_DIR + 1), AP_GET(AP_DIR + 2)};
        GEL_AERO_EMIT(-1, 2, c, aq, nvq, dq, AP_GET(AP_IND), pp.rho, false, false, false);
      } else {
        const double none[3] = {0.0, 0.0, 0.0};
        GEL_AERO_EMIT(-1, 2, c, none, 0.0, none, 0.0, 0.0, false, true, false);
      }
    }
    // ---- position sweeps
#define GEL_AERO_POS_TAIL(c, rp, pq, skip_)                                                          \
  do {                                                                                               \
    double wq_[3], a_[3];                                                                            \
    GEL_AERO_NEED_EA((pq).inv_p, (pq).wn, (pq).we);                                                  \
    wind_eci_or_calm(rp, ea, (pq).sl, (pq).cl, (pq).inv_p, (pq).wn, (pq).we, wq_);                 \
    const double vq_[3] = {xb[4 * M + 3 * xi] * P.uv, xb[4 * M + 3 * xi + 1] * P.uv, xb[4 * M + 3 * xi + 2] * P.uv}; \
    const double nv2_ = aero_vair2(rp, vq_, wq_, a_);                                                \
    const double dd_[3] = {AP_GET(AP_DIR), AP_GET(AP_DIR + 1), AP_GET(AP_DIR + 2)};                  \
    GEL_AERO_EMIT(0, 3, c, a_, nv2_, dd_, AP_GET(AP_IND), (pq).rho, false, false, skip_);                  \
  } while (0)
    const unsigned mine = ROLES ? ((sw == 0) ? 0u : (1u << (sw - 1))) : 7u;   // this wavefront's position sweeps
    unsigned todo = P.fd_recompute ? mine : 0u;   // sweeps with a lane the difference form does not cover (wave-uniform)
    unsigned bad = P.fd_recompute ? 7u : 0u;      // this lane's sweeps among them: only these take the recomputed values
    if (!P.fd_recompute) {
      // the position / velocity / quaternion sweeps as copies of their loop bodies (constant columns and directions): 164 VGPRs,
      // -1.5 % launch time at B = 16384 against the rolled loops (three alternating runs each)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (!((mine >> c) & 1u)) continue;
        asm volatile("" ::: "memory");
        // the scaled position is formed where it is used (fresh_product: not carried across the trips), the velocity read again
        const double r[3] = {fresh_product(re[0], P.up), fresh_product(re[1], P.up), fresh_product(re[2], P.up)};
        double rp[3];
#pragma unroll
        for (int d = 0; d < 3; d++) rp[d] = (d == c) ? (re[d] + dx) * P.up : r[d];
        const double dlt = (c == 0) ? rp[0] - r[0] : ((c == 1) ? rp[1] - r[1] : rp[2] - r[2]);   // exact
        PosPart pq;
        const bool okp = pos_delta(r, c, dlt, pp, pc, tb, pq);
        if (__builtin_amdgcn_ballot_w64(!okp) != 0) { todo |= 1u << c; if (!okp) bad |= 1u << c; }
        GEL_AERO_POS_TAIL(c, rp, pq, !okp);
      }
    }
    if (todo) {   // the chain once more on the perturbed position (like the reference), kept by the lanes that need it
      asm volatile("" ::: "memory");
#pragma unroll 1
      for (int c = 0; c < 3; c++) {
        if (!((todo >> c) & 1u)) continue;
        double rp[3];
#pragma unroll
        for (int d = 0; d < 3; d++) rp[d] = ((d == c) ? xb[M + 3 * xi + d] + dx : xb[M + 3 * xi + d]) * P.up;
        const PosPart pf = pos_part<false, NoSink, false>(rp, tb, 0.0);
        GEL_AERO_POS_TAIL(c, rp, pf, !((bad >> c) & 1u));
      }
    }
#undef GEL_AERO_POS_TAIL
    asm volatile("" ::: "memory");   // the light sweeps read their inputs again
    // ---- velocity sweeps: only the air-relative velocity changes
#pragma unroll
    for (int c = (ROLES && sw != 0) ? 3 : 0; c < 3; c++) {
      double vp[3], a[3];
      const double r[3] = {xb[M + 3 * xi] * P.up, xb[M + 3 * xi + 1] * P.up, xb[M + 3 * xi + 2] * P.up};
#pragma unroll
      for (int d = 0; d < 3; d++) vp[d] = ((d == c) ? xb[4 * M + 3 * xi + d] + dx : xb[4 * M + 3 * xi + d]) * P.uv;
      const double wc[3] = {AP_GET(AP_W), AP_GET(AP_W + 1), AP_GET(AP_W + 2)};
      const double dc[3] = {AP_GET(AP_DIR), AP_GET(AP_DIR + 1), AP_GET(AP_DIR + 2)};
      const double nv2 = aero_vair2(r, vp, wc, a);
      GEL_AERO_EMIT(3, 3, c, a, nv2, dc, AP_GET(AP_IND), AP_GET(AP_RHO), false, false, false);
    }
    // ---- quaternion sweeps: only the body axis changes
    if (need_alpha && !(ROLES && sw != 0)) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        double qp[4], dp[3];
#pragma unroll
        for (int d = 0; d < 4; d++) qp[d] = (d == c) ? xb[7 * M + 4 * xi + d] + dx : xb[7 * M + 4 * xi + d];
        thrust_dir(qp, dp);
        const double indp = frsqrt(fmax(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2], 1.0e-300));
        const double ac[3] = {AP_GET(AP_A0), AP_GET(AP_A0 + 1), AP_GET(AP_A0 + 2)};
        GEL_AERO_EMIT(6, 4, c, ac, AP_GET(AP_NV2), dp, indp, AP_GET(AP_RHO), true, false, false);
      }
    }
  }
#undef GEL_AERO_EMIT
#undef GEL_AERO_NEED_EA
#undef AP_AIDX
#undef AP_GET
#undef AP_SET
  if (!(fabs(chk) <= 1.79769313486231570815e308)) *(volatile int32_t*)P.flag = 1;  // every writer stores the same 1
}

}  // namespace gel
