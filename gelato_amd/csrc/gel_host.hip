// gel_host.hip -- the core of the host side: the thread's message, the pattern walker, the tables and the steps of
// gel_problem_create, the describe calls, the one-vector and host-batch evaluation paths, the shard and full-layout
// device forms (3.2), the caller-owned streams (3.11), the launch-limit checks and the entry points that take no handle.  The other
// host files hold one feature each: gel_host_fd.hip, gel_host_constraints.hip, gel_host_mesh.hip, gel_host_flight.hip,
// gel_host_jprod.hip, gel_host_montecarlo.hip and gel_host_lgr.hip; what they share is gel_host_handle.h (the handle and what makes
// HIP calls) and gel_host_internal.h (no HIP).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "gel_host_handle.h"

// the calling thread's message: g_err, fail() and gel_last_error stay together in this file (no thread_local crosses a translation unit)
namespace gelhost {
namespace {
thread_local std::string g_err;
}
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace gelhost
using namespace gelhost;

// ---- what the other host files call (declared in gel_host_handle.h) ----
namespace gelhost {

// Walks all 13 blocks in the reference's emission order (lib/con_dynamics.py:66-113,
// 155-213,292-496,536-632).  k is the index inside the block.
// Compact slots: see gel_eval_kernel.h (kSlotPT ...).  Layout of a phase's K * n node values: 64-node chunk major,
// [chunk][slot][node of the chunk] -- everything one wavefront writes is one contiguous block (a [slot][n] layout makes a
// wavefront of a phase above 64 nodes write 512 bytes out of every n * 8: measured 8 % slower on 12 x 128).  The per-phase
// scalar sits behind them at voff + K * n.
static inline int64_t compact_index(const HostPhase& h, int slot, int j) {
  const int j0 = j & ~63, w = std::min(64, h.n - j0);
  return h.voff + (int64_t)j0 * h.K + (int64_t)slot * w + (j - j0);
}
void walk_pattern(const gel_problem& P, const Visitor& vis) {
  const int S = (int)P.ph.size();
  int64_t k[GEL_NUM_BLOCKS] = {0};
  auto cs = [&](const HostPhase& h, int slot, int j) { return compact_index(h, slot, j); };
  for (int i = 0; i < S; i++) {
    const HostPhase& h = P.ph[i];
    const int n = h.n, ua = h.ua, xa = h.xa;
    const int64_t scalar = h.voff + (int64_t)h.K * n;  // pos/velocity diagonal value of this phase
    auto Dji = [&](int j, int c) { return h.D[(size_t)j * (n + 1) + c]; };
    // ---- group 0: mass ----
    if (h.engine_on) {
      for (int j = 0; j < n; j++)
        for (int c = 0; c <= n; c++) vis(0, k[0]++, ua + j, xa + c, 0, Dji(j, c), -1);
      const double a = -h.massflow / P.um * P.ut / 2.0, b = h.massflow / P.um * P.ut / 2.0;
      for (int j = 0; j < n; j++) vis(1, k[1]++, ua + j, i, 0, a, -1);
      for (int j = 0; j < n; j++) vis(1, k[1]++, ua + j, i + 1, 0, b, -1);
    } else {
      for (int j = 0; j < n; j++) vis(0, k[0]++, ua + j, xa, 0, -1.0, -1);
      for (int j = 0; j < n; j++) vis(0, k[0]++, ua + j, xa + 1 + j, 0, 1.0, -1);
    }
    // ---- group 1: position ----
    for (int ki = 0; ki < 3; ki++)
      for (int j = 0; j < n; j++)
        for (int c = 0; c <= n; c++) vis(2, k[2]++, 3 * (ua + j) + ki, 3 * (xa + c) + ki, 0, Dji(j, c), -1);
    for (int jj = 0; jj < 3 * n; jj++) vis(3, k[3]++, 3 * ua + jj, 3 * (xa + 1) + jj, 1, 0, scalar);
    for (int jj = 0; jj < 3 * n; jj++) vis(4, k[4]++, 3 * ua + jj, i, 1, 0, cs(h, 0 + jj % 3, jj / 3));
    for (int jj = 0; jj < 3 * n; jj++) vis(4, k[4]++, 3 * ua + jj, i + 1, 2, 0, cs(h, 0 + jj % 3, jj / 3));
    // ---- group 2: velocity ----
    for (int j = 0; j < n; j++)
      for (int c = 0; c < 3; c++) vis(5, k[5]++, 3 * (ua + j) + c, xa + 1 + j, 1, 0, cs(h, 3 + c, j));
    for (int kk = 0; kk < 3; kk++)
      for (int j = 0; j < n; j++)
        for (int c = 0; c < 3; c++) vis(6, k[6]++, 3 * (ua + j) + c, 3 * (xa + 1 + j) + kk, 1, 0, cs(h, 6 + 3 * kk + c, j));
    for (int ki = 0; ki < 3; ki++)
      for (int kj = 0; kj < 3; kj++)
        for (int j = 0; j < n; j++)
          for (int cc = 0; cc <= n; cc++) {
            const double dv = (ki == kj) ? Dji(j, cc) : 0.0;
            if (cc == j + 1 && h.air_fd)
              vis(7, k[7]++, 3 * (ua + j) + ki, 3 * (xa + cc) + kj, 1, 0, cs(h, h.s_vv + 3 * kj + ki, j));
            else
              vis(7, k[7]++, 3 * (ua + j) + ki, 3 * (xa + cc) + kj, 0, dv, -1);
          }
    for (int kk = 0; kk < 4; kk++)
      for (int j = 0; j < n; j++)
        for (int c = 0; c < 3; c++) vis(8, k[8]++, 3 * (ua + j) + c, 4 * (xa + 1 + j) + kk, 1, 0, cs(h, h.s_vq + 3 * kk + c, j));
    // t0 column, then tf column: two sweeps when the velocity / time derivatives are finite differences
    // (reference_area > 0), else the tf column is the exact negative of the t0 column (:478-480)
    for (int jj = 0; jj < 3 * n; jj++) vis(9, k[9]++, 3 * ua + jj, i, 1, 0, cs(h, h.s_vt + jj % 3, jj / 3));
    for (int jj = 0; jj < 3 * n; jj++)
      vis(9, k[9]++, 3 * ua + jj, i + 1, h.t_fd ? 1 : 2, 0, cs(h, h.s_vt + (h.t_fd ? 3 : 0) + jj % 3, jj / 3));
    // ---- group 3: quaternion ----
    if (h.hold) {
      for (int jj = 0; jj < 4 * n; jj++) vis(10, k[10]++, 4 * ua + jj, 4 * xa + jj % 4, 0, -1.0, -1);
      for (int jj = 0; jj < 4 * n; jj++) vis(10, k[10]++, 4 * ua + jj, 4 * (xa + 1) + jj, 0, 1.0, -1);
    } else {
      for (int j = 0; j < n; j++)
        for (int c = 0; c < 4; c++)
          for (int cc = 0; cc <= n; cc++)
            for (int kk = 0; kk < 4; kk++) {
              // on the block diagonal dq_c/dq_kk is a finite difference only where dq_c contains q_kk
              // (src/pybind_dynamics.cpp:94-106: rows {0,1} x columns {2,3} and rows {2,3} x columns {0,1});
              // elsewhere the reference's difference is exactly zero and the entry is D[j][j+1] or 0
              if (cc == j + 1 && ((c < 2) != (kk < 2))) {
                if (h.q_fd)
                  vis(10, k[10]++, 4 * (ua + j) + c, 4 * (xa + cc) + kk, 1, 0, cs(h, h.s_qq + 2 * kk + (c & 1), j));
                else {
                  // closed form (dq is linear in q): two values per node, A = omega_y S / 2 (slot s_qq) and B = omega_z S / 2
                  // (s_qq + 1), S = (tf - to) unit_t / 2; entry (c, kk) = -d(dq_c)/d(q_kk) S  (src/pybind_dynamics.cpp:94-106)
                  static const int which[4][4] = {{-1, -1, 0, 1}, {-1, -1, 1, 0}, {0, 1, -1, -1}, {1, 0, -1, -1}};   // [c][kk]
                  static const int sign[4][4] = {{0, 0, +1, +1}, {0, 0, -1, +1}, {-1, +1, 0, 0}, {-1, -1, 0, 0}};
                  vis(10, k[10]++, 4 * (ua + j) + c, 4 * (xa + cc) + kk, sign[c][kk] > 0 ? 1 : 2, 0, cs(h, h.s_qq + which[c][kk], j));
                }
              } else
                vis(10, k[10]++, 4 * (ua + j) + c, 4 * (xa + cc) + kk, 0, (c == kk) ? Dji(j, cc) : 0.0, -1);
            }
      for (int kk = 0; kk < 2; kk++)
        for (int j = 0; j < n; j++)
          for (int c = 0; c < 4; c++) {
            if (h.q_fd)
              vis(11, k[11]++, 4 * (ua + j) + c, 2 * (ua + j) + kk, 1, 0, cs(h, h.s_qq + 8 + 4 * kk + c, j));
            else {
              // closed form (dq is linear in u): slots s_qq + 2 .. 5 hold C_0' = -C_0, C_1, C_2, C_3 with C_i = unit_u (pi/180) q_i S / 2
              // (the first negated so that every slot has a positive use); entry (c, kk) = -d(dq_c)/d(u_kk) S
              static const int which[2][4] = {{2, 3, 0, 1}, {3, 2, 1, 0}};          // [kk][c]: which C
              static const int sign[2][4] = {{+1, +1, -1, -1}, {+1, -1, +1, -1}};
              const int w = which[kk][c];
              const int sg = (w == 0) ? -sign[kk][c] : sign[kk][c];                  // slot of C_0 stores -C_0
              vis(11, k[11]++, 4 * (ua + j) + c, 2 * (ua + j) + kk, sg > 0 ? 1 : 2, 0, cs(h, h.s_qq + 2 + w, j));
            }
          }
      const int s_qt = h.s_qq + (h.q_fd ? 16 : 6);
      for (int jj = 0; jj < 4 * n; jj++) vis(12, k[12]++, 4 * ua + jj, i, 1, 0, cs(h, s_qt + jj % 4, jj / 4));
      for (int jj = 0; jj < 4 * n; jj++) vis(12, k[12]++, 4 * ua + jj, i + 1, 2, 0, cs(h, s_qt + jj % 4, jj / 4));
    }
  }
}

// The stream a device-form entry point launches on: the caller's (remembered for drain) or, for NULL, the handle's own.
hipStream_t stream_of(gel_problem* p, void* stream) {
  if (!stream) return p->stream.get();
  return p->caller_stream = (hipStream_t)stream;
}
// Before device memory that launches read or write is released or replaced (a reconfiguration, a new shard plan, a workspace that
// grows): wait for the handle's own stream AND for the last caller-owned stream, so that nothing in flight still uses the old block.
hipError_t drain(gel_problem* p) {
  if (p->stream.get())
    if (const hipError_t e = hipStreamSynchronize(p->stream.get())) return e;
  if (p->caller_stream)
    if (const hipError_t e = hipStreamSynchronize(p->caller_stream)) return e;
  return hipSuccess;
}
// A host-form call that found the device's non-finite flag set clears it and WAITS for the clear, as gel_sync does: a launch that
// the caller enqueues on a stream of its own right after the return must not have its flag wiped by a memset that runs late.
hipError_t clear_flag(gel_problem* p, hipStream_t s) {
  if (const hipError_t e = hipMemsetAsync(p->d_flag.get(), 0, 4, s)) return e;
  return hipStreamSynchronize(s);
}

// Launches that stage the tables pass no launch attribute: a workgroup of theirs may take gel::kLaunchMaxLds bytes.  The host decides
// with the launchers' own sizes (gel_launch.h, gel_mesh.h), before anything is enqueued; the device is never asked.
// lds_room: the table doubles that fit beside `rest` doubles of other LDS (padded: the rest starts at an even double)
size_t lds_room(size_t rest, bool padded) {
  const size_t cap = gel::kLaunchMaxLds / sizeof(double);
  const size_t r = rest < cap ? cap - rest : 0;
  return padded ? (r & ~(size_t)1) : r;
}
// GEL_OK, or GEL_ERR_ARG with the table doubles asked for and those that fit; `staged` = the doubles the tables take in the launch
int check_launch_lds(const char* what, size_t lds_bytes, size_t asked, size_t staged, bool padded) {
  if (lds_bytes <= gel::kLaunchMaxLds) return GEL_OK;
  const size_t room = lds_room(lds_bytes / sizeof(double) - staged, padded);
  return fail(GEL_ERR_ARG, std::string(what) + ": the tables take " + std::to_string(asked) + " doubles of LDS, " + std::to_string(room) +
                               " fit beside the launch's own (64 KB per workgroup): fewer wind or CA rows");
}
int check_table_launches(int Kw, int Kc) {
  const size_t T = gel::staged_table_doubles(Kw, Kc), Tp = gel::padded_table_doubles(Kw, Kc);
  if (int rc = check_launch_lds("fused kernel", gel::eval_lds_bytes_max(Kw, Kc), T, Tp, true)) return rc;
  return check_launch_lds("aero kernels", gel::aero_lds_bytes(Kw, Kc), T, Tp, true);
}

int need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(GEL_ERR_HIP, "no HIP device: the engine has no CPU fallback");
  return GEL_OK;
}

// ---- pipelined host batch ----
constexpr size_t kPipeBytes = (size_t)16 << 20;  // staging per slot and direction

// memcpy on a few threads: one core moves ~10 GB/s, PCIe delivers 2-5x that
void par_copy(void* dst, const void* src, size_t bytes) {
  const size_t kMin = (size_t)2 << 20;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const size_t nt = std::min<size_t>(std::min<size_t>(4, hw), bytes / kMin);
  if (nt <= 1) { std::memcpy(dst, src, bytes); return; }
  std::vector<std::thread> th;
  const size_t per = ((bytes / nt) + 63) & ~(size_t)63;
  for (size_t t = 1; t < nt; t++) {
    const size_t off = t * per, len = (t + 1 == nt) ? bytes - off : per;
    th.emplace_back([=] { std::memcpy((char*)dst + off, (const char*)src + off, len); });
  }
  std::memcpy(dst, src, per);
  for (auto& t : th) t.join();
}

int ensure_slots(gel_problem* p) {
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (p->pipe_evals) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  const size_t per_eval = 8 * (size_t)std::max<int64_t>(p->dims.num_var_entries, 1);
  const int cap = (int)std::max<size_t>(1, kPipeBytes / per_eval);
  const size_t nx = (size_t)cap * p->dims.num_vars, nr = (size_t)cap * 11 * p->dims.N, nj = (size_t)cap * std::max<int64_t>(1, p->dims.num_var_entries);
  gel_problem::Slot fresh[2];   // all or nothing: a failure frees what was made, and the next call starts from scratch
  for (auto& sl : fresh) {
    const bool ok = sl.d_x.reserve(nx) == hipSuccess && sl.d_res.reserve(nr) == hipSuccess && sl.d_jv.reserve(nj) == hipSuccess &&
                    sl.d_flag.reserve(1) == hipSuccess && hipMemset(sl.d_flag.get(), 0, 4) == hipSuccess &&
                    sl.h_x.reserve(nx) == hipSuccess && sl.h_res.reserve(nr) == hipSuccess && sl.h_jv.reserve(nj) == hipSuccess &&
                    sl.h_flag.reserve(1) == hipSuccess && sl.stream.create() == hipSuccess;
    if (!ok) return fail(GEL_ERR_ALLOC, "staging slots: allocation failed");
    *sl.h_flag.get() = 0;
  }
  for (int i = 0; i < 2; i++) p->slot[i] = std::move(fresh[i]);
  p->pipe_evals = cap;
  return GEL_OK;
}

}  // namespace gelhost

namespace {

// doubles of one phase's block in the host table: sigma | Lx | Lu | I
inline size_t mesh_block_doubles(int n) { return (size_t)(n + 1) * (1 + (n + 1) + n + (n + 1)); }

int64_t phase_block_nnz(const HostPhase& h, int blk) {
  const int64_t n = h.n;
  switch (blk) {
    case 0: return h.engine_on ? n * (n + 1) : 2 * n;
    case 1: return h.engine_on ? 2 * n : 0;
    case 2: return 3 * n * (n + 1);
    case 3: return 3 * n;
    case 4: return 6 * n;
    case 5: return 3 * n;
    case 6: return 9 * n;
    case 7: return 9 * n * (n + 1);
    case 8: return 12 * n;
    case 9: return 6 * n;
    case 10: return h.hold ? 8 * n : 16 * n * (n + 1);
    case 11: return h.hold ? 0 : 8 * n;
    default: return h.hold ? 0 : 8 * n;
  }
}

#define NO_EXACT(p, what)                                                                                                   \
  do {                                                                                                                      \
    if ((p)->exact) return fail(GEL_ERR_ARG, what " has no exact-Jacobian form (handle created with GEL_FLAG_EXACT_DEFECT_JAC)"); \
  } while (0)

int ensure_capacity(gel_problem* p, int B) {
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (B <= p->capB) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(drain(p));   // the old staging blocks go: nothing in flight may still use them
  p->capB = 0;   // until every buffer below has grown
  const size_t nx = (size_t)B * p->dims.num_vars, nr = (size_t)B * 11 * p->dims.N, nj = (size_t)B * std::max<int64_t>(1, p->dims.num_var_entries);
  HIPCHK(p->d_x.reserve(nx)); HIPCHK(p->d_res.reserve(nr)); HIPCHK(p->d_jv.reserve(nj));
  HIPCHK(p->h_x.reserve(nx)); HIPCHK(p->h_res.reserve(nr)); HIPCHK(p->h_jv.reserve(nj));
  p->capB = B;
  return GEL_OK;
}

// Wait for a short launch.  Round 5, measured on the one-vector path (three resident processes taking turns, same box): polling
// hipStreamQuery 39.1 us per Engine.eval, hipStreamSynchronize 37.3 us, the same after hipSetDeviceFlags(hipDeviceScheduleSpin) 37.0 us
// -- this runtime's synchronise spins on the completion signal itself before it sleeps, and a query is a full API call per poll
// (rounds 1-4 measured the opposite on an earlier runtime and polled).  GEL_WAIT_MODE=0 restores the polling loop (measurement switch).
// Self-signalling one-vector launches: the kernel's last workgroup stores the launch's sequence number to a pinned host word once
// every workgroup's results are visible system-wide (gel_eval_kernel.h signal_done); the host spins on that word instead of waiting
// for the end-of-kernel signal, which the runtime hands over 4 us later at 6 x 64 (29 -> 25 us launch-to-results).  The stream still
// holds the kernel's tail; whatever is launched next on it is ordered behind.  GEL_DONE_FLAG=0: off (measurement switch).
static bool done_flag_on() {
  static const bool on = [] { const char* e = getenv("GEL_DONE_FLAG"); return !e || atoi(e) != 0; }();
  return on;
}
static void arm_done(gel_problem* p, gel::ProblemDev& dv) {
  if (!p->done.d_ctr.get() || !p->done.h_word.get() || !done_flag_on()) return;
  dv.done_ctr = p->done.d_ctr.get();
  dv.done_flag = const_cast<int32_t*>(p->done.h_word.get());
  dv.done_seq = ++p->done.seq;
}
static hipError_t spin_wait(hipStream_t s);
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::this_thread::yield();
#endif
}
static hipError_t wait_done(gel_problem* p, const gel::ProblemDev& dv) {
  if (dv.done_flag) {
    // Spin budget: a few times what this handle's launches have taken so far (floor 200 us, ceiling 5 ms) -- with several resident
    // processes taking turns on the GPU, or a preempted queue, a fixed 5 ms burnt a core per call before the runtime's wait was
    // taken anyway.  A launch that never signals (it should not happen) falls back to that wait as well.
    const auto t0 = std::chrono::steady_clock::now();
    const auto budget = std::chrono::microseconds(std::min<long long>(5000, std::max<long long>(200, 8 * p->done.ema_us)));
    for (unsigned it = 1;; it++) {
      if (*p->done.h_word.get() == dv.done_seq) {
        std::atomic_thread_fence(std::memory_order_acquire);
        const long long us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        p->done.ema_us = (3 * p->done.ema_us + us + 3) / 4;
        return hipSuccess;
      }
      cpu_relax();
      if ((it & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > budget) break;
    }
    p->done.ema_us = std::min<long long>(5000, 2 * p->done.ema_us + 50);   // the wait outlasted the budget: a longer one next time
  }
  return spin_wait(p->stream.get());
}

static hipError_t spin_wait(hipStream_t s) {
  static const int mode = [] { const char* e = getenv("GEL_WAIT_MODE"); return e ? atoi(e) : 1; }();
  if (mode) return hipStreamSynchronize(s);
  hipError_t q;
  while ((q = hipStreamQuery(s)) == hipErrorNotReady) {}
  return q;
}

// The engine's own full COO value array and residual vector in pinned host memory (one-vector latency path): the constants are
// laid down here, once; the COO-direct kernel and the host's scatter of the few entries left to it rewrite the x-dependent ones.
int ensure_full(gel_problem* p) {
  if (p->h_full.get() && p->cb_res.get() && p->cb_x[0].get() && p->cb_x[1].get()) return GEL_OK;
  HIPCHK(hipSetDevice(p->device));
  // each buffer on its own: a failed allocation leaves the others as they are and the next call tries again (no half-made set is
  // ever handed out: gel_pinned_buffers and the zero-copy checks only run after this function has returned GEL_OK)
  if (!p->h_full.get()) HIPCHK(p->h_full.upload(p->cval));
  HIPCHK(p->cb_res.reserve((size_t)11 * p->dims.N));
  for (auto& b : p->cb_x) HIPCHK(b.reserve((size_t)p->dims.num_vars));
  return GEL_OK;
}
// GEL_NO_COO_DIRECT=1 (measurement switch): the compact layout + the host scatter of every x-dependent entry, as before round 5
bool coo_direct(const gel_problem* p) {
  static const bool off = [] { const char* e = getenv("GEL_NO_COO_DIRECT"); return e && atoi(e) != 0; }();
  return !off && !p->coo_tab.empty() && p->d_coo.get() != nullptr;
}
// After a COO-direct evaluation: the entries the kernel left to the host (the diagonal of the dense velocity block, the pairs of the
// dense quaternion block: 11 of a node's 49 slots) go from the compact vector into the engine's array; a caller that brought its
// own array gets the all-x-dependent blocks as whole copies and the same few scattered entries.
void finish_full(gel_problem* p, double* vals_full, int fill) {
  auto rest = [&](double* out) {
    for (const gel_problem::Run& r : p->rest_runs) {
      double* d = out + r.dst0;
      const double* v = p->h_jv.get() + r.src0;
      if (r.sign > 0) for (int64_t k = 0; k < r.len; k++) d[k * r.dstride] = v[k * r.sstride];
      else for (int64_t k = 0; k < r.len; k++) d[k * r.dstride] = -v[k * r.sstride];
    }
  };
  rest(p->h_full.get());
  if (vals_full == p->h_full.get()) return;
  if (fill) std::memcpy(vals_full, p->cval.data(), p->cval.size() * 8);
  for (int b : {3, 4, 5, 6, 8, 9, 11, 12})
    std::memcpy(vals_full + p->block_off[b], p->h_full.get() + p->block_off[b], (size_t)(p->block_off[b + 1] - p->block_off[b]) * 8);
  rest(vals_full);
}

// run B evals from host x; leaves results in the pinned staging buffers (res_to: where the kernel writes the residual vector
// of a one-vector call -- the handle's staging buffer or the pinned vector the caller named; coo: COO-direct Jacobian output)
int run_host(gel_problem* p, int B, const double* x, bool want_res, bool want_jac, double* res_to = nullptr, bool* coo_io = nullptr) {
  const bool coo = coo_io && *coo_io;
  if (coo_io) *coo_io = false;   // set again where the mode is really used (the zero-copy branch)
  int rc = ensure_capacity(p, B);
  if (rc) return rc;
  HIPCHK(hipSetDevice(p->device));
  const size_t nx = (size_t)B * p->dims.num_vars, nr = (size_t)B * 11 * p->dims.N, nj = (size_t)B * p->dims.num_var_entries;
  // a one-vector call whose x IS one of the handle's pinned decision-vector buffers (gel_pinned_buffers) is read in place
  const bool x_pinned = B == 1 && p->cb_x[0].get() && (x == p->cb_x[0].get() || x == p->cb_x[1].get());
  if (!x_pinned) std::memcpy(p->h_x.get(), x, nx * 8);
  const double* const xin = x_pinned ? x : p->h_x.get();
  if ((nx + (want_res ? nr : 0) + (want_jac ? nj : 0)) * 8 <= kZeroCopyBytes) {
    // Small calls (the optimiser's one-vector callbacks): the kernel reads x from and writes its results
    // to the pinned staging buffers itself -- one launch and one synchronise instead of launch + four
    // copy commands (measured 91 -> see DESIGN.md 5, B = 1).  The non-finite flag is a plain store of 1,
    // so it may live in host memory too.
    gel::ProblemDev dv = p->dev;
    dv.flag = p->h_flag.get();
    // COO-direct output exists in the latency form only: a problem of more than 256 work items takes a cooperative form even for one
    // vector (gel::eval_form) and keeps the compact path
    if (coo && !p->exact && B == 1 && want_jac && gel::eval_form(dv, 1, want_res, true).split) { dv.coo_full = p->h_full.get(); dv.coo = p->d_coo.get(); *coo_io = true; }
    dv.split_vel = 1;   // a whole evaluation: every part of every work item is in this launch
    // the latency form tells the host itself when its results are there (not when the exact kernel follows it)
    if (!(p->exact && want_jac) && gel::eval_form(dv, B, want_res, want_jac).split) arm_done(p, dv);
    HIPCHK(launch_defects(p, dv, B, xin, want_res ? (res_to ? res_to : p->h_res.get()) : nullptr, want_jac ? p->h_jv.get() : nullptr, p->stream.get()));
    HIPCHK(wait_done(p, dv));
    if (*p->h_flag.get()) { *p->h_flag.get() = 0; return GEL_NONFINITE; }
    return GEL_OK;
  }
  hipStream_t s = p->stream.get();
  HIPCHK(hipMemcpyAsync(p->d_x.get(), xin, nx * 8, hipMemcpyHostToDevice, s));
  HIPCHK(launch_defects(p, p->dev, B, p->d_x.get(), want_res ? p->d_res.get() : nullptr, want_jac ? p->d_jv.get() : nullptr, s));
  if (want_res) HIPCHK(hipMemcpyAsync(p->h_res.get(), p->d_res.get(), nr * 8, hipMemcpyDeviceToHost, s));
  if (want_jac && nj) HIPCHK(hipMemcpyAsync(p->h_jv.get(), p->d_jv.get(), nj * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(p->h_flag.get(), p->d_flag.get(), 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (want_res && res_to) std::memcpy(res_to, p->h_res.get(), nr * 8);
  if (*p->h_flag.get()) {
    *p->h_flag.get() = 0;
    HIPCHK(clear_flag(p, s));
    return GEL_NONFINITE;
  }
  return GEL_OK;
}

// B evals from / to pageable host arrays in sub-batches: while sub-batch i runs (H2D, kernel, D2H on its
// slot's stream), the host retires sub-batch i-1 of the other slot (pinned -> caller) and stages i+1.
// Is this host pointer page-locked memory the runtime knows (its own pinned allocations or hipHostRegister, e.g. a torch tensor made with
// pin_memory = True)?  Then the copy engines read and write it directly and the staging copy through the handle's slots is skipped.
static bool is_pinned(const void* ptr) {
  if (!ptr) return false;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

int run_host_pipelined(gel_problem* p, int B, const double* x, double* res, double* jvar) {
  int rc = ensure_slots(p);
  if (rc) return rc;
  HIPCHK(hipSetDevice(p->device));
  // page-locked caller buffers (all that are given): no staging copies on the host at all -- H2D straight from x, D2H straight into
  // res / jvar, sub-batch by sub-batch on the two slots' streams; the host only waits
  const bool direct = is_pinned(x) && (!res || is_pinned(res)) && (!jvar || is_pinned(jvar));
  const int cap = p->pipe_evals;
  const size_t nv = (size_t)p->dims.num_vars, nr = (size_t)11 * p->dims.N, nj = (size_t)p->dims.num_var_entries;
  const int nsub = (B + cap - 1) / cap;
  int status = GEL_OK;
  auto retire = [&](gel_problem::Slot& sl) -> int {
    if (!sl.count) return GEL_OK;
    HIPCHK(hipStreamSynchronize(sl.stream.get()));
    if (*sl.h_flag.get()) {
      *sl.h_flag.get() = 0;
      HIPCHK(hipMemsetAsync(sl.d_flag.get(), 0, 4, sl.stream.get()));
      status = GEL_NONFINITE;
    }
    if (!direct) {
      if (sl.res) par_copy(res + (size_t)sl.first * nr, sl.h_res.get(), (size_t)sl.count * nr * 8);
      if (sl.jac && nj) par_copy(jvar + (size_t)sl.first * nj, sl.h_jv.get(), (size_t)sl.count * nj * 8);
    }
    sl.count = 0;
    return GEL_OK;
  };
  for (int i = 0; i < nsub; i++) {
    gel_problem::Slot& sl = p->slot[i & 1];
    if ((rc = retire(sl))) break;
    const int64_t first = (int64_t)i * cap;
    const int count = (int)std::min<int64_t>(cap, B - first);
    if (!direct) par_copy(sl.h_x.get(), x + (size_t)first * nv, (size_t)count * nv * 8);
    sl.first = first; sl.count = count; sl.res = res != nullptr; sl.jac = jvar != nullptr;
    gel::ProblemDev dv = p->dev;
    dv.flag = sl.d_flag.get();
    const double* const hx = direct ? x + (size_t)first * nv : sl.h_x.get();
    double* const hres = direct ? res + (size_t)first * nr : sl.h_res.get();
    double* const hjv = direct ? jvar + (size_t)first * nj : sl.h_jv.get();
    hipStream_t s = sl.stream.get();
    if (hipMemcpyAsync(sl.d_x.get(), hx, (size_t)count * nv * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_defects(p, dv, count, sl.d_x.get(), res ? sl.d_res.get() : nullptr, jvar ? sl.d_jv.get() : nullptr, s) != hipSuccess ||
        (res && hipMemcpyAsync(hres, sl.d_res.get(), (size_t)count * nr * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        (jvar && nj && hipMemcpyAsync(hjv, sl.d_jv.get(), (size_t)count * nj * 8, hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipMemcpyAsync(sl.h_flag.get(), sl.d_flag.get(), 4, hipMemcpyDeviceToHost, s) != hipSuccess) {
      rc = fail(GEL_ERR_HIP, "pipelined batch: enqueue failed");
      break;
    }
  }
  // drain both slots (also after an error, so that nothing is left in flight)
  for (int k = 0; k < 2; k++) {
    const int r2 = retire(p->slot[(nsub + k) & 1]);
    if (!rc) rc = r2;
  }
  return rc ? rc : status;
}

void scatter_full(const gel_problem* p, const double* jv, double* vals_full, int fill) {
  if (fill) std::memcpy(vals_full, p->cval.data(), p->cval.size() * 8);
  // the index map is a few hundred constant-stride runs: no index loads, predictable strides
  for (const gel_problem::Run& r : p->var_runs) {
    double* d = vals_full + r.dst0;
    const double* v = jv + r.src0;
    if (r.sign > 0) for (int64_t k = 0; k < r.len; k++) d[k * r.dstride] = v[k * r.sstride];
    else for (int64_t k = 0; k < r.len; k++) d[k * r.dstride] = -v[k * r.sstride];
  }
}

}  // namespace

namespace gel {
void fill_atmosphere_table(double* atm) {
  // src/Air.cpp:31-45
  const double lmb[11] = {-0.0065, 0.0, 0.001, 0.0028, 0.0, -0.0028, -0.002, 0.0, 0.0025, 0.012, 0.012};
  const double tmb[11] = {288.15, 216.65, 216.65, 228.65, 270.65, 270.65, 214.65, 186.8673, 186.8673, 240.0, 360.0};
  const double pb[11] = {101325.0, 22632.0, 5474.9, 868.02, 110.91, 66.939, 3.9564, 0.37338, 0.15381, 7.1042e-3, 2.5382e-3};
  const double mb[11] = {28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9644, 28.9522, 28.89, 27.27, 26.20};
  for (int k = 0; k < 11; k++) {
    atm[k] = lmb[k];
    atm[11 + k] = tmb[k];
    atm[22 + k] = pb[k];
    atm[33 + k] = 8314.32 / mb[k];  // Rstar / mb[k], src/Air.cpp:67
    // the two per-layer constants of Air::pressure (src/Air.cpp:93-97), reference operation order
    const double R = atm[33 + k], g0 = 9.80665;
    atm[44 + k] = (std::fabs(lmb[k]) > 1.0e-6) ? (-g0 / lmb[k] / R) : 0.0;
    atm[55 + k] = g0 / R;
    static const double hb[11] = {0.0, 11000.0, 20000.0, 32000.0, 47000.0, 51000.0, 71000.0, 86000.0, 91000.0, 110000.0, 120000.0};
    atm[66 + k] = hb[k];  // src/Air.cpp:29-30
    atm[77 + k] = 1.0 / tmb[k];
  }
}

// validates the interpolation tables (np.interp's precondition; the bracket search and the tabulated slopes of
// the device lookup rely on >= 2 rows and strictly increasing abscissae) -- nullptr if fine, else the complaint
const char* check_tables(const double* wind, int Kw, const double* ca, int Kc) {
  if (!wind || !ca || Kw < 2 || Kc < 2) return "wind and CA tables need at least two rows";
  for (int k = 1; k < Kw; k++)
    if (!(wind[3 * k] > wind[3 * (k - 1)])) return "wind table altitudes must increase strictly";
  for (int k = 1; k < Kc; k++)
    if (!(ca[2 * k] > ca[2 * (k - 1)])) return "CA table Mach numbers must increase strictly";
  return nullptr;
}

// rows [K][w] followed by the slopes (y[k+1][c] - y[k][c]) / (x[k+1] - x[k]) of every interval, c = 1..w-1
void append_rows_and_slopes(std::vector<double>& rows_out, std::vector<double>& slopes_out, const double* tab, int K, int w) {
  rows_out.insert(rows_out.end(), tab, tab + (size_t)K * w);
  for (int k = 0; k + 1 < K; k++)
    for (int c = 1; c < w; c++)
      slopes_out.push_back((tab[(size_t)(k + 1) * w + c] - tab[(size_t)k * w + c]) / (tab[(size_t)(k + 1) * w] - tab[(size_t)k * w]));
}

// atmosphere | wind rows | CA rows | wind slopes | CA slopes  (gel_physics.h table_doubles())
std::vector<double> build_tables(const double* wind, int Kw, const double* ca, int Kc) {
  std::vector<double> t(kAtmTableDoubles), slopes;
  fill_atmosphere_table(t.data());
  append_rows_and_slopes(t, slopes, wind, Kw, 3);
  append_rows_and_slopes(t, slopes, ca, Kc, 2);
  t.insert(t.end(), slopes.begin(), slopes.end());
  return t;
}
}  // namespace gel

namespace {

// ---- the steps of gel_problem_create, in the order it takes them; each returns a gel_* status ----
int create_validate(const gel_problem_desc* d) {
  if (d->num_sections < 1 || !d->num_nodes || !d->thrust || !d->massflow || !d->reference_area || !d->nozzle_area ||
      !d->engine_on || !d->attitude_hold || !d->wind_table || !d->ca_table || d->wind_rows < 2 || d->ca_rows < 2)
    return fail(GEL_ERR_ARG, "incomplete problem description");
  if (!(d->dx > 0.0)) return fail(GEL_ERR_ARG, "dx must be positive");
  // the exact Jacobian fills the default compact layout (closed-form t0 / tf and quaternion slots); the aero rows it leaves to
  // finite differences keep their difference form, which needs a step of at most 1 m
  if ((d->flags & GEL_FLAG_EXACT_DEFECT_JAC) &&
      ((d->flags & GEL_FLAG_FD_RECOMPUTE) || !(std::fabs(d->dx * d->unit_position) <= 1.0)))
    return fail(GEL_ERR_ARG, "GEL_FLAG_EXACT_DEFECT_JAC cannot be combined with GEL_FLAG_FD_RECOMPUTE (nor with |dx * unit_position| > 1)");
  // the exact aero gradients fill the default layout (t columns as exact zeros, no t columns in the records' part A)
  if ((d->flags & GEL_FLAG_EXACT_AERO_JAC) &&
      ((d->flags & GEL_FLAG_FD_RECOMPUTE) || !(std::fabs(d->dx * d->unit_position) <= 1.0)))
    return fail(GEL_ERR_ARG, "GEL_FLAG_EXACT_AERO_JAC cannot be combined with GEL_FLAG_FD_RECOMPUTE (nor with |dx * unit_position| > 1)");
  if (const char* why = gel::check_tables(d->wind_table, d->wind_rows, d->ca_table, d->ca_rows)) return fail(GEL_ERR_ARG, why);
  // every evaluation goes through the fused and the aero launches; their limit (1792 table doubles) is below that of the launches
  // that keep nothing behind the tables (exact forms, propagation, output table: 8192), which therefore need no check of their own
  if (int rc = check_table_launches(d->wind_rows, d->ca_rows)) return rc;
  for (int i = 0; i < d->num_sections; i++)
    if (d->num_nodes[i] < 2) return fail(GEL_ERR_ARG, "every phase needs >= 2 LGR nodes (nodes_LGR requires n >= 2)");
  // device == GEL_DEVICE_NONE: a host-only handle (dims, LGR data, sparsity pattern, constant values,
  // work partition) that can describe the problem but never evaluate it -- there is no CPU fallback.
  if (d->device != GEL_DEVICE_NONE) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
      return fail(GEL_ERR_HIP, "no HIP device: the engine has no CPU fallback");
    if (d->device < 0 || d->device >= ndev) return fail(GEL_ERR_ARG, "device ordinal out of range");
  }
  return GEL_OK;
}

// flags, units, the phases' layout and the dims
int create_layout(gel_problem* p, const gel_problem_desc* d) {
  p->device = d->device;
  p->um = d->unit_mass; p->up = d->unit_position; p->uv = d->unit_velocity; p->uu = d->unit_u; p->ut = d->unit_t;
  p->dx = d->dx;
  // Position sweeps in exact-difference form and the t0 / tf columns in closed form (gel_rhs_parts.h pos_delta, gel_eval_kernel.h),
  // unless the caller asks for the reference's recomputing sweeps or the step dx * unit_position is beyond the 1 m the
  // truncated series of the difference form are sized for (the reference's own dx = 1e-8 gives 0.064 m).
  p->fd_recompute = ((d->flags & GEL_FLAG_FD_RECOMPUTE) != 0) || !(std::fabs(d->dx * d->unit_position) <= 1.0);
  p->exact = (d->flags & GEL_FLAG_EXACT_DEFECT_JAC) != 0;
  p->exact_aero = (d->flags & GEL_FLAG_EXACT_AERO_JAC) != 0;
  p->exact_rows = (d->flags & GEL_FLAG_EXACT_ROWS_JAC) != 0;
  const char* fused = std::getenv("GEL_AERO_FUSED");
  p->aero_fused = !(fused && fused[0] == '0');
  p->barC20 = (d->barC20 == 0.0) ? -0.484165371736e-3 : d->barC20;
  const int S = d->num_sections;
  int N = 0;
  size_t offD = 0, offT = 0;
  int64_t V = 0;
  p->ph.resize(S);
  for (int i = 0; i < S; i++) {
    HostPhase& h = p->ph[i];
    h.n = d->num_nodes[i]; h.ua = N; h.xa = N + i; N += h.n;
    h.thrust = d->thrust[i]; h.massflow = d->massflow[i]; h.area = d->reference_area[i]; h.nozzle = d->nozzle_area[i];
    h.air = (h.area != 0.0); h.air_fd = (h.area > 0.0);
    h.t_fd = h.air_fd && p->fd_recompute;
    h.engine_on = d->engine_on[i] != 0; h.hold = d->attitude_hold[i] != 0;
    h.s_vv = 15; h.s_vq = h.air_fd ? 24 : 15; h.s_vt = h.s_vq + 12; h.s_qq = h.s_vt + (h.t_fd ? 6 : 3);
    h.q_fd = !h.hold && p->fd_recompute;   // quaternion kinematics: finite differences (20 slots) or closed form (10)
    h.K = h.s_qq + (h.hold ? 0 : (h.q_fd ? 20 : 10));
    h.voff = V; V += (int64_t)h.K * h.n + 1;  // node slots + the phase's pos/velocity diagonal scalar
    const size_t nd = (size_t)h.n * (h.n + 1);
    if (d->D && d->tau) {
      h.D.assign(d->D + offD, d->D + offD + nd);
      h.tau.assign(d->tau + offT, d->tau + offT + h.n);
    } else {
      int same = -1;
      for (int j = 0; j < i; j++) if (p->ph[j].n == h.n) { same = j; break; }
      if (same >= 0) { h.D = p->ph[same].D; h.tau = p->ph[same].tau; }
      else lgr_diffmat_ld(h.n, h.D, h.tau);
    }
    offD += nd; offT += h.n;
  }
  const int M = N + S;
  gel_dims& dm = p->dims;
  dm.S = S; dm.N = N; dm.M = M; dm.num_vars = 11 * M + 2 * N + S + 1;
  dm.num_rows[0] = N; dm.num_rows[1] = 3 * N; dm.num_rows[2] = 3 * N; dm.num_rows[3] = 4 * N;
  const int64_t T = S + 1;
  const int64_t rk[13] = {1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4};
  const int64_t ck[13] = {M, T, 3 * M, 3 * M, T, M, 3 * M, 3 * M, 4 * M, T, 4 * M, 2 * N, T};
  int64_t tot = 0;
  for (int b = 0; b < GEL_NUM_BLOCKS; b++) {
    int64_t s = 0;
    for (int i = 0; i < S; i++) s += phase_block_nnz(p->ph[i], b);
    dm.block_nnz[b] = s;
    dm.block_shape[b][0] = rk[b] * N;
    dm.block_shape[b][1] = ck[b];
    p->block_off[b] = tot;
    tot += s;
  }
  p->block_off[GEL_NUM_BLOCKS] = tot;
  dm.total_nnz = tot;
  dm.num_var_entries = V;
  {
    // A_min = read x once + write the residual once + write every x-dependent value the reference
    // computes once: V_ref = sum over phases of n * (9 [pos] + 39 | 30 [vel with | without velocity / time FD] + 32 [free
    // attitude]).  The engine's compact vector holds the DISTINCT values among them (stored_bytes).
    int64_t Vref = 0;
    for (int i = 0; i < S; i++) Vref += (int64_t)p->ph[i].n * (9 + (p->ph[i].air_fd ? 39 : 30) + (p->ph[i].hold ? 0 : 32));
    dm.algorithmic_bytes = 8 * ((int64_t)dm.num_vars + 11 * (int64_t)N + Vref);
    dm.stored_bytes = 8 * (11 * (int64_t)N + V);
  }
  return GEL_OK;
}

// the gather map (constants, sources, first use of every compact slot) and its constant-stride runs
int create_gather_map(gel_problem* p, const gel_problem_desc*) {
  const int S = p->dims.S;
  const int64_t V = p->dims.num_var_entries, tot = p->dims.total_nnz;
  // pattern-derived host arrays
  p->cval.assign((size_t)tot, 0.0);
  p->src.assign((size_t)tot, -1);
  p->var_idx.assign((size_t)V, -1);
  struct Ref { int64_t slot, f; int kind; int64_t occ; };
  std::vector<Ref> refs;
  walk_pattern(*p, [&](int blk, int64_t k, int32_t, int32_t, int kind, double cv, int64_t slot) {
    const int64_t f = p->block_off[blk] + k;
    if (kind == 0) { p->cval[(size_t)f] = cv; return; }
    p->src[(size_t)f] = (kind == 1) ? (int32_t)slot : (int32_t)(-2 - slot);
    if (kind == 1 && p->var_idx[(size_t)slot] < 0) p->var_idx[(size_t)slot] = f;
    refs.push_back({slot, f, kind, 0});
  });
  for (int64_t s = 0; s < V; s++)
    if (p->var_idx[(size_t)s] < 0) return fail(GEL_ERR_ARG, "internal: compact slot without a COO entry");
  {
    // The gather map as constant-stride runs for the host scatter.  A per-node slot is used once or twice (a t0
    // column and its negated tf column): its k-th use over consecutive nodes is one run.  A phase scalar is used
    // 3n times: its uses in full order are one run with source stride 0.
    std::vector<char> is_scalar((size_t)V, 0);
    for (int i = 0; i < S; i++) is_scalar[(size_t)(p->ph[i].voff + (int64_t)p->ph[i].K * p->ph[i].n)] = 1;
    std::stable_sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return a.slot < b.slot; });
    for (size_t i = 0; i < refs.size(); i++)
      refs[i].occ = (i > 0 && refs[i - 1].slot == refs[i].slot && !is_scalar[(size_t)refs[i].slot]) ? refs[i - 1].occ + 1 : 0;
    std::stable_sort(refs.begin(), refs.end(), [](const Ref& a, const Ref& b) { return a.occ < b.occ; });  // (occ, slot, f)
    for (size_t i = 0; i < refs.size();) {
      size_t j = i + 1;
      const bool sc = is_scalar[(size_t)refs[i].slot] != 0;
      const int64_t ds = (j < refs.size()) ? refs[j].f - refs[i].f : 1;
      while (j < refs.size() && refs[j].kind == refs[i].kind && refs[j].occ == refs[i].occ &&
             refs[j].slot == refs[j - 1].slot + (sc ? 0 : 1) && refs[j].f - refs[j - 1].f == ds &&
             (is_scalar[(size_t)refs[j].slot] != 0) == sc)
        j++;
      p->var_runs.push_back({refs[i].f, ds, refs[i].slot, sc ? 0 : 1, (int64_t)(j - i), refs[i].kind == 1 ? 1.0 : -1.0});
      i = j;
    }
  }
  return GEL_OK;
}

int create_coo_direct(gel_problem* p, const gel_problem_desc*) {
  const int S = p->dims.S;
  const int64_t tot = p->dims.total_nnz;
  if (!p->fd_recompute) {
    // COO-direct groups: where the runs of the all-x-dependent blocks start in the full value vector (the emission order of
    // walk_pattern() = the reference's), checked against the gather map itself -- any surprise switches the mode off
    int64_t kb[GEL_NUM_BLOCKS] = {0};
    std::vector<int32_t> tab((size_t)8 * S, -1);
    bool ok = tot < (int64_t)1 << 31;
    for (int i = 0; i < S && ok; i++) {
      const HostPhase& h = p->ph[i];
      const int n = h.n;
      auto at = [&](int b) { return p->block_off[b] + kb[b]; };
      int32_t* t = &tab[(size_t)8 * i];
      t[0] = (int32_t)at(3); t[1] = (int32_t)at(4); t[2] = (int32_t)at(5); t[3] = (int32_t)at(6); t[4] = (int32_t)at(8); t[5] = (int32_t)at(9);
      t[6] = h.hold ? -1 : (int32_t)at(11); t[7] = h.hold ? -1 : (int32_t)at(12);
      // spot checks against the map: node j, component c of group g sits at t[g] + w (n k + j) + c and takes slot(g, k, c) of node j
      auto expect = [&](int64_t f, int slot, int j, int sign) {
        const int64_t s = compact_index(h, slot, j);
        ok = ok && f >= 0 && f < tot && p->src[(size_t)f] == (sign > 0 ? (int32_t)s : (int32_t)(-2 - s));
      };
      for (int j : {0, n - 1})
        for (int c = 0; c < 3; c++) {
          ok = ok && p->src[(size_t)(t[0] + 3 * j + c)] == (int32_t)(h.voff + (int64_t)h.K * n);
          expect(t[1] + 3 * j + c, 0 + c, j, +1); expect(t[1] + 3 * (n + j) + c, 0 + c, j, -1);
          expect(t[2] + 3 * j + c, 3 + c, j, +1);
          for (int k = 0; k < 3; k++) expect(t[3] + 3 * (n * k + j) + c, 6 + 3 * k + c, j, +1);
          for (int k = 0; k < 4; k++) expect(t[4] + 3 * (n * k + j) + c, h.s_vq + 3 * k + c, j, +1);
          expect(t[5] + 3 * j + c, h.s_vt + c, j, +1); expect(t[5] + 3 * (n + j) + c, h.s_vt + c, j, -1);
        }
      if (!h.hold)
        for (int j : {0, n - 1})
          for (int c = 0; c < 4; c++) {
            // quat/u: the kernel's COO form writes {C2, C3, -C0, -C1 | C3, -C2, C1, -C0} with slots s_qq + 2 .. 5 = -C0, C1, C2, C3
            static const int which[2][4] = {{2, 3, 0, 1}, {3, 2, 1, 0}}, sg[2][4] = {{+1, +1, -1, -1}, {+1, -1, +1, -1}};
            for (int k = 0; k < 2; k++) expect(t[6] + 4 * (n * k + j) + c, h.s_qq + 2 + which[k][c], j, which[k][c] == 0 ? -sg[k][c] : sg[k][c]);
            expect(t[7] + 4 * j + c, h.s_qq + 6 + c, j, +1); expect(t[7] + 4 * (n + j) + c, h.s_qq + 6 + c, j, -1);
          }
      for (int b = 0; b < GEL_NUM_BLOCKS; b++) kb[b] += phase_block_nnz(h, b);
    }
    if (ok) {
      p->coo_tab = tab;
      for (const gel_problem::Run& r : p->var_runs) {
        const int b = (int)(std::upper_bound(p->block_off, p->block_off + GEL_NUM_BLOCKS + 1, r.dst0) - p->block_off) - 1;
        if (b == 7 || b == 10) p->rest_runs.push_back(r);
      }
    }
  }
  return GEL_OK;
}

int create_mesh_host(gel_problem* p, const gel_problem_desc* d) {
  const int S = p->dims.S;
  {
    // collocation error estimate: every phase's block, built aside and committed once all are there (a phase that repeats an
    // earlier one's n and tau repeats its block)
    std::vector<double> mh, blk;
    std::vector<size_t> hoff;
    int32_t npts = 0;
    bool fits = true;
    for (int i = 0; i < S; i++) { npts += p->ph[i].n + 1; fits = fits && p->ph[i].n + 1 <= gel::kMeshMaxThreads; }
    for (int i = 0; fits && i < S; i++) {
      const HostPhase& h = p->ph[i];
      int same = -1;
      for (int j = 0; j < i; j++) if (p->ph[j].n == h.n && p->ph[j].tau == h.tau) { same = j; break; }
      hoff.push_back(mh.size());
      if (same >= 0) blk.assign(mh.begin() + hoff[same], mh.begin() + hoff[same] + mesh_block_doubles(h.n));
      else if (mesh_matrices_ld(h.tau, blk)) return fail(GEL_ERR_ARG, "collocation error tables: singular integration matrix");
      mh.insert(mh.end(), blk.begin(), blk.end());
    }
    p->mesh.host = std::move(mh);
    p->mesh.hoff = std::move(hoff);
    p->mesh.npts = npts;
    for (int i = 0; fits && i < S; i++) p->mesh.lds_max = std::max(p->mesh.lds_max, gel::mesh_lds_bytes(d->wind_rows, d->ca_rows, p->ph[i].n));
  }
  return GEL_OK;
}

// the Jacobian products' tables and the work partition
int create_products_host(gel_problem* p, const gel_problem_desc* d) {
  const int S = p->dims.S;
  p->dev.Kw = d->wind_rows; p->dev.Kc = d->ca_rows;
  if (const char* e = build_jprod_tables(*p)) return fail(GEL_ERR_ARG, e);
  if (const char* e = getenv("GEL_JPROD_THREADS")) { if (atoi(e) == 256) p->jp.threads = 256; }   // host-only handles report it too
  for (int i = 0; i < S; i++)
    for (int j0 = 0; j0 < p->ph[i].n; j0 += 64) p->chunk_phase.push_back(i);
  return GEL_OK;
}

// the device's phase records, the work items and D in the matrix pipe's feed orders, built on the host and uploaded
int create_device_tables(gel_problem* p, const gel_problem_desc* d) {
  const int S = p->dims.S, N = p->dims.N;
  std::vector<gel::PhaseDev> dph(S);
  std::vector<int32_t> node_phase(N);
  std::vector<double> Dt, tau;
  for (int i = 0; i < S; i++) {
    const HostPhase& h = p->ph[i];
    gel::PhaseDev& q = dph[i];
    q.n = h.n; q.ua = h.ua; q.xa = h.xa; q.air = h.air; q.air_fd = h.air_fd; q.t_fd = h.t_fd; q.q_fd = h.q_fd; q.engine_on = h.engine_on; q.hold = h.hold;
    q.K = h.K; q.s_vv = h.s_vv; q.s_vq = h.s_vq; q.s_vt = h.s_vt; q.s_qq = h.s_qq;
    q.doff = (int32_t)Dt.size(); q.toff = (int32_t)tau.size(); q.voff = h.voff;
    q.thrust = h.thrust; q.massflow = h.massflow; q.area = h.area; q.nozzle = h.nozzle;
    q.mf_um = -h.massflow / p->um;
    for (int c = 0; c <= h.n; c++)
      for (int j = 0; j < h.n; j++) Dt.push_back(h.D[(size_t)j * (h.n + 1) + c]);
    tau.insert(tau.end(), h.tau.begin(), h.tau.end());
    for (int j = 0; j < h.n; j++) node_phase[h.ua + j] = i;
  }
  const std::vector<double> tables = gel::build_tables(d->wind_table, d->wind_rows, d->ca_table, d->ca_rows);
  // Work items, and D laid out the way the matrix pipe consumes it.  A operand of v_mfma_f64_16x16x4_f64:
  // lane l holds A[row l & 15][k l >> 4]; a wavefront covers 64 nodes = 4 row tiles, and k-step ks covers
  // columns 4 ks .. 4 ks + 3 of D.  Dsw[((item_off + ks) * 64 + l) * 4 + t] = D[j0 + 16 t + (l & 15)][4 ks + (l >> 4)]
  // (0 beyond column n; rows beyond the phase repeat its last row: computed, never read back), so that one lane
  // fetches its four tile operands of a k-step with a single 32-byte access at a fixed stride.
  std::vector<int4> chunks;
  std::vector<double> Dsw, Dst;
  for (int i = 0; i < S; i++) {
    const HostPhase& h = p->ph[i];
    const int n = h.n, ksteps = (n + 4) >> 2;
    for (int j0 = 0; j0 < n; j0 += 64) {
      // .w: where the chunk stands in its phase's run and how long the run is (the cooperative launch order keeps the chunks
      // of a phase and a group of vectors together, gel_eval_kernel.h)
      chunks.push_back(make_int4(i, j0, (int)(Dsw.size() / 4), ((j0 / 64) << 16) | ((h.n + 63) / 64)));
      for (int ks = 0; ks < ksteps; ks++)
        for (int l = 0; l < 64; l++)
          for (int t = 0; t < 4; t++) {
            const int k = 4 * ks + (l >> 4), row = std::min(j0 + 16 * t + (l & 15), n - 1);
            Dsw.push_back(k <= n ? h.D[(size_t)row * (n + 1) + k] : 0.0);
          }
      // Dst[((item_off + ks) * 4 + t) * 64 + l]: the same element, row tile t contiguous over the lanes
      for (int ks = 0; ks < ksteps; ks++)
        for (int t = 0; t < 4; t++)
          for (int l = 0; l < 64; l++) {
            const int k = 4 * ks + (l >> 4), row = std::min(j0 + 16 * t + (l & 15), n - 1);
            Dst.push_back(k <= n ? h.D[(size_t)row * (n + 1) + k] : 0.0);
          }
    }
  }

  // launch order of a whole evaluation: aerodynamic phases (the long chain, 4x + sweeps) before NoAir
  // ones, free attitude before held -- the same weights gelato_amd/parallel.py balances shards with
  std::vector<int4> sorted_chunks = chunks;
  auto weight = [&](const int4& c) { return (p->ph[c.x].air ? 10.0 : 1.5) + (p->ph[c.x].hold ? 0.0 : 0.5); };
  std::stable_sort(sorted_chunks.begin(), sorted_chunks.end(), [&](const int4& a, const int4& b) { return weight(a) > weight(b); });

  // the phase-ordered list serves shard launches over ARBITRARY work-item ranges: no runs there
  std::vector<int4> shard_chunks = chunks;
  for (int4& c : shard_chunks) c.w = 1;
  HIPCHK(p->d_chunks.upload(shard_chunks)); HIPCHK(p->d_chunks_sorted.upload(sorted_chunks)); HIPCHK(p->d_Dsw.upload(Dsw));
  HIPCHK(p->d_Dst.upload(Dst)); HIPCHK(p->d_phases.upload(dph)); HIPCHK(p->d_node_phase.upload(node_phase)); HIPCHK(p->d_Dt.upload(Dt));
  HIPCHK(p->d_tau.upload(tau)); HIPCHK(p->d_tables.upload(tables)); HIPCHK(p->d_cval.upload(p->cval)); HIPCHK(p->d_src.upload(p->src));
  {
    std::vector<int32_t> vdst, vsrc;
    for (size_t i = 0; i < p->src.size(); i++)
      if (p->src[i] != -1) { vdst.push_back((int32_t)i); vsrc.push_back(p->src[i]); }
    p->nvar_entries = (int32_t)vdst.size();
    if (!vdst.empty()) { HIPCHK(p->d_vdst.upload(vdst)); HIPCHK(p->d_vsrc.upload(vsrc)); }
    std::vector<int32_t> vline;
    for (int32_t d : vdst)
      if (vline.empty() || vline.back() != d / 8) vline.push_back(d / 8);
    p->nvar_lines = (int32_t)vline.size();
    if (!vline.empty()) HIPCHK(p->d_vline.upload(vline));
    if (!p->coo_tab.empty()) HIPCHK(p->d_coo.upload(p->coo_tab));
  }
  {
    // one-phase sub-problems for the phase-by-phase forward difference (gel_jac_fd)
    std::vector<gel::PhaseDev> sub = dph;
    std::vector<int4> subchunks = chunks;
    std::vector<int32_t> colmap;
    int c0 = 0;
    for (int i = 0; i < S; i++) {
      sub[i].ua = 0; sub[i].xa = 0; sub[i].voff = 0;
      p->jfd.sub_chunk0.push_back(c0);
      int cnt = 0;
      while (c0 + cnt < (int)chunks.size() && chunks[c0 + cnt].x == i) { subchunks[c0 + cnt].x = 0; cnt++; }
      p->jfd.sub_nchunks.push_back(cnt);
      c0 += cnt;
      p->jfd.sub_col0.push_back((int32_t)colmap.size());
      phase_columns(p, i, colmap);
    }
    HIPCHK(p->jfd.d_subphases.upload(sub)); HIPCHK(p->jfd.d_subchunks.upload(subchunks)); HIPCHK(p->jfd.d_colmap.upload(colmap));
  }
  if (p->d_flag.reserve(1) != hipSuccess || hipMemset(p->d_flag.get(), 0, 4) != hipSuccess ||
      p->done.d_ctr.reserve(1) != hipSuccess || hipMemset(p->done.d_ctr.get(), 0, 4) != hipSuccess || p->done.h_word.reserve(1) != hipSuccess ||
      p->h_flag.reserve(1) != hipSuccess || p->stream.create() != hipSuccess)
    return fail(GEL_ERR_HIP, "device allocation failed");
  *p->h_flag.get() = 0;
  return GEL_OK;
}

int create_problem_dev(gel_problem* p, const gel_problem_desc* d) {
  const int S = p->dims.S, N = p->dims.N, M = p->dims.M;
  const int64_t V = p->dims.num_var_entries;
  const gel_dims& dm = p->dims;
  gel::ProblemDev& dv = p->dev;
  dv.S = S; dv.N = N; dv.M = M; dv.nvars = dm.num_vars; dv.Kw = d->wind_rows; dv.Kc = d->ca_rows; dv.V = V;
  dv.phases = p->d_phases.get(); dv.node_phase = p->d_node_phase.get(); dv.Dt = p->d_Dt.get(); dv.tau = p->d_tau.get();
  dv.tables = p->d_tables.get(); dv.flag = p->d_flag.get();
  dv.nchunks = (int32_t)p->chunk_phase.size(); dv.chunks = p->d_chunks_sorted.get(); dv.Dsw = p->d_Dsw.get(); dv.Dst = p->d_Dst.get();
  dv.park_off = (int32_t)gel::padded_table_doubles(d->wind_rows, d->ca_rows);
  int nmax = 0;
  for (int i = 0; i < S; i++) nmax = std::max(nmax, p->ph[i].n);
  {
    // D.X path.  fp64 MFMA and fp64 VALU instructions share the SIMD's fp64 datapath on this part (measured: their busy
    // times add up), so the matrix pipe is not free throughput; what it buys is fewer issue slots and the
    // cooperative form: four decision vectors side by side (44 of 48 tile columns used, a quarter of the D traffic), and --
    // when every phase fits 32 lanes -- two decision vectors per wavefront, which no wavefront dot-product form offers.
    // Same-box A/B, evals/s at B = 32768, matrix pipe vs VALU (tools/dx_paths.sh): 3x8 97.2 M vs 53.3 M, 3x16 77.7 M vs
    // 49.1 M, 3x32 55.2 M vs 40.1 M, 6x64 13.9 M vs 12.7 M; residual-only 3x8 265 M vs 163 M, 3x16 217 M vs 129 M, 3x32
    // 161 M vs 91 M, 6x64 31.3 M vs 21.4 M.  Between 33 and 63 nodes per phase the matrix pipe wins as well (one vector per
    // wavefront).  Only a mesh that mixes phases above 32 nodes with many tiny ones would prefer the dot-products; none
    // of the reference's configurations does.  GEL_FLAG_DX_VALU / _MFMA force a path.
    dv.use_mfma = (d->flags & GEL_FLAG_DX_VALU) ? 0 : 1;
    dv.pack = (nmax <= 32) && !(d->flags & GEL_FLAG_NO_PACK);
    dv.longp = (nmax >= gel::kLongPhaseFrom) ? 1 : 0;
  }
  dv.fd_recompute = p->fd_recompute ? 1 : 0;
  // measured (same box): 3 x 32 +4 % (fused and residual-only), 6 x 64 -1..2 %: only the small-phase meshes, whose rows share most lines
  dv.vmajor = (nmax <= 32 && !(d->flags & GEL_FLAG_ITEM_MAJOR)) ? 1 : 0;
  dv.um = p->um; dv.up = p->up; dv.uv = p->uv; dv.uu = p->uu; dv.ut = p->ut; dv.dx = p->dx; dv.barC20 = p->barC20;
  dv.inv_uv = 1.0 / p->uv; dv.inv_dx = 1.0 / p->dx; dv.kpt = p->uv * p->ut / 2.0 / p->up; dv.hT = p->ut * 0.5;
  return GEL_OK;
}

int create_mesh_device(gel_problem* p, const gel_problem_desc* d) {
  const int S = p->dims.S;
  if (!p->mesh.hoff.empty()) {
    // the estimate's device tables: each phase's matrices transposed (point index fastest), LDS per workgroup of vpb vectors
    std::vector<double> mat;
    std::vector<gel::MeshPhaseDev> mph(S);
    int32_t pt0 = 0;
    for (int i = 0; i < S; i++) {
      const int n = p->ph[i].n, P = n + 1;
      const double* hb = p->mesh.host.data() + p->mesh.hoff[i];
      const double *sg = hb, *Lx = sg + P, *Lu = Lx + (size_t)P * P, *I = Lu + (size_t)P * n;
      gel::MeshPhaseDev& q = mph[i];
      q.n = n; q.pt0 = pt0; q.pad = 0;
      q.vpb = gel::kMeshMaxThreads / P;                                                   // the vectors the workgroup has lanes for ...
      q.vpb = std::min(q.vpb, gel::mesh_vectors_that_fit(d->wind_rows, d->ca_rows, n));   // ... and LDS (gel::mesh_vectors_per_group)
      pt0 += P;
      q.lx = (int64_t)mat.size();
      for (int k = 0; k < P; k++) for (int l = 0; l < P; l++) mat.push_back(Lx[(size_t)l * P + k]);
      q.lu = (int64_t)mat.size();
      for (int k = 0; k < n; k++) for (int l = 0; l < P; l++) mat.push_back(Lu[(size_t)l * n + k]);
      q.it = (int64_t)mat.size();
      for (int k = 0; k < P; k++) for (int l = 0; l < P; l++) mat.push_back(I[(size_t)l * P + k]);
      q.sg = (int64_t)mat.size();
      for (int l = 0; l < P; l++) mat.push_back(sg[l]);
      q.lds = (int64_t)gel::mesh_lds_bytes(d->wind_rows, d->ca_rows, n);
    }
    HIPCHK(p->mesh.d_mat.upload(mat)); HIPCHK(p->mesh.d_ph.upload(mph));
    p->mesh.ph = std::move(mph);
    gel::MeshDev& md = p->mesh.dev;
    md.S = S; md.npts = p->mesh.npts; md.ph = p->mesh.d_ph.get(); md.mat = p->mesh.d_mat.get(); md.vp = p->uv / p->up;
  }
  return GEL_OK;
}

int create_products_device(gel_problem* p, const gel_problem_desc*) {
  HIPCHK(p->jp.d_it.upload(p->jp.it)); HIPCHK(p->jp.d_dt.upload(p->jp.dt)); HIPCHK(p->jp.d_ph.upload(p->jp.ph));
  p->jp.dev.ph = p->jp.d_ph.get(); p->jp.dev.it = p->jp.d_it.get(); p->jp.dev.dt = p->jp.d_dt.get();
  return GEL_OK;
}

}  // namespace

extern "C" {

const char* gel_last_error(void) { return g_err.c_str(); }
const char* gel_version(void) { return "gelato_amd 0.1 (gfx950, fp64)"; }

int gel_problem_create(const gel_problem_desc* d, gel_problem** out) {
  if (!d || !out) return fail(GEL_ERR_ARG, "null argument");
  if (int rc = create_validate(d)) return rc;
  std::unique_ptr<gel_problem> p(new gel_problem());   // released to the caller on success only
  gel_problem* const h = p.get();
  if (int rc = create_layout(h, d)) return rc;
  if (int rc = create_gather_map(h, d)) return rc;
  if (int rc = create_coo_direct(h, d)) return rc;
  if (int rc = create_mesh_host(h, d)) return rc;
  if (int rc = create_products_host(h, d)) return rc;
  if (p->device == GEL_DEVICE_NONE) {
    p->dev.nchunks = (int32_t)p->chunk_phase.size();
    *out = p.release();
    return GEL_OK;
  }

  // device side
  if (hipSetDevice(p->device) != hipSuccess) return fail(GEL_ERR_HIP, "hipSetDevice failed");
  if (int rc = create_device_tables(h, d)) return rc;
  if (int rc = create_problem_dev(h, d)) return rc;
  if (int rc = create_mesh_device(h, d)) return rc;
  if (int rc = create_products_device(h, d)) return rc;
  *out = p.release();
  return GEL_OK;
}

int gel_problem_destroy(gel_problem* p) {
  delete p;
  return GEL_OK;
}

int gel_problem_dims(const gel_problem* p, gel_dims* out) {
  if (!p || !out) return fail(GEL_ERR_ARG, "null argument");
  *out = p->dims;
  return GEL_OK;
}

int gel_problem_D(const gel_problem* p, int32_t i, double* D) {
  if (!p || !D || i < 0 || i >= (int)p->ph.size()) return fail(GEL_ERR_ARG, "Index out of range");
  std::memcpy(D, p->ph[i].D.data(), p->ph[i].D.size() * 8);
  return GEL_OK;
}

int gel_problem_tau(const gel_problem* p, int32_t i, double* tau) {
  if (!p || !tau || i < 0 || i >= (int)p->ph.size()) return fail(GEL_ERR_ARG, "Index out of range");
  std::memcpy(tau, p->ph[i].tau.data(), p->ph[i].tau.size() * 8);
  return GEL_OK;
}

int gel_pattern(const gel_problem* p, int32_t block, int32_t* rows, int32_t* cols) {
  if (!p || !rows || !cols || block < 0 || block >= GEL_NUM_BLOCKS) return fail(GEL_ERR_ARG, "bad block");
  walk_pattern(*p, [&](int blk, int64_t k, int32_t r, int32_t c, int, double, int64_t) {
    if (blk == block) { rows[k] = r; cols[k] = c; }
  });
  return GEL_OK;
}

int gel_pattern_all(const gel_problem* p, int32_t* rows_full, int32_t* cols_full) {
  if (!p || !rows_full || !cols_full) return fail(GEL_ERR_ARG, "null argument");
  walk_pattern(*p, [&](int blk, int64_t k, int32_t r, int32_t c, int, double, int64_t) {
    rows_full[p->block_off[blk] + k] = r;
    cols_full[p->block_off[blk] + k] = c;
  });
  return GEL_OK;
}

int gel_const_values(const gel_problem* p, double* vals_full) {
  if (!p || !vals_full) return fail(GEL_ERR_ARG, "null argument");
  std::memcpy(vals_full, p->cval.data(), p->cval.size() * 8);
  return GEL_OK;
}

int gel_var_index(const gel_problem* p, int64_t* idx) {
  if (!p || !idx) return fail(GEL_ERR_ARG, "null argument");
  std::memcpy(idx, p->var_idx.data(), p->var_idx.size() * 8);
  return GEL_OK;
}

int gel_full_source(const gel_problem* p, int32_t* src) {
  if (!p || !src) return fail(GEL_ERR_ARG, "null argument");
  std::memcpy(src, p->src.data(), p->src.size() * sizeof(int32_t));
  return GEL_OK;
}

int gel_pinned_buffers(gel_problem* p, double** res, double** vals_full, double** x0, double** x1) {
  if (!p) return fail(GEL_ERR_ARG, "null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (int rc = ensure_full(p)) return rc;
  if (res) *res = p->cb_res.get();
  if (vals_full) *vals_full = p->h_full.get();
  if (x0) *x0 = p->cb_x[0].get();
  if (x1) *x1 = p->cb_x[1].get();
  return GEL_OK;
}

int gel_eval_residual(gel_problem* p, const double* x, double* res) {
  if (!p || !x || !res) return fail(GEL_ERR_ARG, "null argument");
  const bool own = p->cb_res.get() && res == p->cb_res.get();   // the caller named the handle's pinned vector: the kernel writes it, no copy
  const int rc = run_host(p, 1, x, true, false, own ? p->cb_res.get() : nullptr);
  if (rc < 0) return rc;
  if (!own) std::memcpy(res, p->h_res.get(), (size_t)11 * p->dims.N * 8);
  return rc;
}

int gel_eval_jacobian(gel_problem* p, const double* x, double* vals_full, int32_t fill_constants) {
  return gel_eval(p, x, nullptr, vals_full, fill_constants);
}

int gel_eval(gel_problem* p, const double* x, double* res, double* vals_full, int32_t fill_constants) {
  if (!p || !x || !vals_full) return fail(GEL_ERR_ARG, "null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  bool coo = coo_direct(p);
  if (coo) { if (int rc0 = ensure_full(p)) return rc0; }
  const bool own = res && p->cb_res.get() && res == p->cb_res.get();
  const int rc = run_host(p, 1, x, res != nullptr, true, own ? p->cb_res.get() : nullptr, &coo);
  if (rc < 0) return rc;
  if (res && !own) std::memcpy(res, p->h_res.get(), (size_t)11 * p->dims.N * 8);
  if (coo) finish_full(p, vals_full, fill_constants);
  else scatter_full(p, p->h_jv.get(), vals_full, fill_constants);
  return rc;
}

int gel_eval_batch(gel_problem* p, int32_t B, const double* x, double* res, double* jvar) {
  if (!p || !x || B < 1 || (!res && !jvar)) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  // more than one staging slot's worth: sub-batches through the two-slot pipeline
  if ((size_t)B * 8 * (size_t)std::max<int64_t>(p->dims.num_var_entries, 1) > kPipeBytes) return run_host_pipelined(p, B, x, res, jvar);
  const int rc = run_host(p, B, x, res != nullptr, jvar != nullptr);
  if (rc < 0) return rc;
  if (res) std::memcpy(res, p->h_res.get(), (size_t)B * 11 * p->dims.N * 8);
  if (jvar) std::memcpy(jvar, p->h_jv.get(), (size_t)B * p->dims.num_var_entries * 8);
  return rc;
}

int gel_eval_batch_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, void* stream) {
  if (!p || !d_x || B < 1 || (!d_res && !d_jvar)) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(launch_defects(p, p->dev, B, d_x, d_res, d_jvar, stream_of(p, stream)));
  return GEL_OK;
}

int gel_eval_shard_units_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar,
                                int32_t unit_begin, int32_t unit_count, void* stream) {
  if (!p || !d_x || B < 1 || !d_jvar) return fail(GEL_ERR_ARG, "bad argument (the unit form always writes Jacobian values)");
  NO_EXACT(p, "gel_eval_shard_units_device");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  const int32_t total = 4 * (int32_t)p->chunk_phase.size();
  if (unit_begin < 0 || unit_count < 0 || unit_begin + unit_count > total)
    return fail(GEL_ERR_ARG, "unit range out of bounds");
  if (unit_count == 0) return GEL_OK;
  gel::ProblemDev dv = p->dev;
  dv.chunks = p->d_chunks.get();  // unit ids refer to the phase-ordered list
  dv.chunk0 = 0;
  dv.unit0 = unit_begin;
  dv.nunits = unit_count;
  HIPCHK(gel::launch_eval(dv, B, d_x, d_res, d_jvar, stream_of(p, stream)));
  return GEL_OK;
}

int gel_num_chunks(const gel_problem* p, int32_t* nchunks) {
  if (!p || !nchunks) return fail(GEL_ERR_ARG, "null argument");
  *nchunks = (int32_t)p->chunk_phase.size();
  return GEL_OK;
}

int gel_chunk_phase(const gel_problem* p, int32_t* phase) {
  if (!p || !phase) return fail(GEL_ERR_ARG, "null argument");
  std::memcpy(phase, p->chunk_phase.data(), p->chunk_phase.size() * sizeof(int32_t));
  return GEL_OK;
}

int gel_launch_info(const gel_problem* p, int32_t B, int32_t want_res, int32_t want_jac, int32_t* info) {
  if (!p || !info || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  const gel::EvalForm f = gel::eval_form(p->dev, B, want_res != 0, want_jac != 0);
  info[0] = f.jac; info[1] = f.mfma; info[2] = f.split; info[3] = (int32_t)std::min<long long>(f.waves, INT32_MAX);
  info[4] = f.pack;
  return GEL_OK;
}

int gel_unit_owner(const gel_problem* p, int32_t* res_owner, int32_t* jvar_owner) {
  if (!p || !res_owner || !jvar_owner) return fail(GEL_ERR_ARG, "null argument");
  // unit = 4 * work item + part (phase-ordered work items): part 0 writes the residual rows of the item's nodes and
  // every compact value of those nodes except the position-sweep columns of an aerodynamic phase, which parts 1..3
  // write (one column = three slots each); the phase scalar belongs to part 0 of the phase's first work item
  const int N = p->dims.N;
  int item = 0;
  for (size_t i = 0; i < p->ph.size(); i++) {
    const HostPhase& h = p->ph[i];
    for (int j0 = 0; j0 < h.n; j0 += 64, item++) {
      const int j1 = std::min(j0 + 64, h.n);
      for (int j = j0; j < j1; j++) {
        const int g = h.ua + j;
        res_owner[g] = 4 * item;
        for (int c = 0; c < 3; c++) { res_owner[N + 3 * g + c] = 4 * item; res_owner[4 * N + 3 * g + c] = 4 * item; }
        for (int c = 0; c < 4; c++) res_owner[7 * N + 4 * g + c] = 4 * item;
        for (int s = 0; s < h.K; s++) {
          const int part = (h.air && s >= 6 && s < 15) ? 1 + (s - 6) / 3 : 0;
          jvar_owner[compact_index(h, s, j)] = 4 * item + part;
        }
      }
      if (j0 == 0) jvar_owner[h.voff + (int64_t)h.K * h.n] = 4 * item;
    }
  }
  return GEL_OK;
}

// Packed unit-shard exchange: the layout every rank agrees on.  Rank r holds units [unit_begin[r], unit_begin[r + 1]); the block
// of a unit inside its rank's per-vector block: the compact slots it owns as [slot][node of the chunk] (part 0 of an aerodynamic
// phase: all but slots 6 .. 14; part k > 0: slots 6 + 3 (k - 1) .. + 2), the phase scalar behind them (part 0 of a phase's first
// chunk), then (part 0) the residual rows mass | position 3 | velocity 3 | quaternion 4 of the chunk's nodes -- what
// eval_body<.., SPLIT> writes when ProblemDev::shard_width != 0.
int gel_shard_plan(gel_problem* p, int32_t nranks, const int32_t* unit_begin, int64_t* width, int64_t* res_pos, int64_t* jvar_pos) {
  if (!p || nranks < 1 || !unit_begin || !width) return fail(GEL_ERR_ARG, "bad argument");
  const int32_t nunits = 4 * (int32_t)p->chunk_phase.size();
  if (unit_begin[0] != 0 || unit_begin[nranks] != nunits) return fail(GEL_ERR_ARG, "the unit ranges must cover every unit");
  for (int r = 0; r < nranks; r++)
    if (unit_begin[r + 1] < unit_begin[r]) return fail(GEL_ERR_ARG, "the unit ranges must be ordered");
  const int N = p->dims.N;
  const int64_t V = p->dims.num_var_entries;
  std::vector<int64_t> usize(nunits, 0), pos((size_t)11 * N + V, -1);
  std::vector<int32_t> urank(nunits, 0);
  for (int r = 0; r < nranks; r++)
    for (int u = unit_begin[r]; u < unit_begin[r + 1]; u++) urank[u] = r;
  // sizes first (bases need them), then positions
  {
    int item = 0;
    for (const HostPhase& h : p->ph)
      for (int j0 = 0; j0 < h.n; j0 += 64, item++) {
        const int64_t nn = std::min(64, h.n - j0);
        const int skip = h.air ? 9 : 0;
        usize[4 * item] = (int64_t)(h.K - skip) * nn + (j0 == 0 ? 1 : 0) + 11 * nn;
        for (int k = 1; k < 4; k++) usize[4 * item + k] = h.air ? 3 * nn : 0;
      }
  }
  std::vector<int64_t> base(nunits, 0);
  int64_t w = 0;
  for (int r = 0; r < nranks; r++) {
    int64_t off = 0;
    for (int u = unit_begin[r]; u < unit_begin[r + 1]; u++) { base[u] = off; off += usize[u]; }
    w = std::max(w, off);
  }
  w = (w + 1) & ~(int64_t)1;   // 16-byte multiples: every rank's slice and every vector's block start aligned
  {
    int item = 0;
    for (const HostPhase& h : p->ph)
      for (int j0 = 0; j0 < h.n; j0 += 64, item++) {
        const int nn = std::min(64, h.n - j0);
        const int skip = h.air ? 9 : 0;
        const int64_t nj = (int64_t)(h.K - skip) * nn + (j0 == 0 ? 1 : 0);
        const int u0 = 4 * item;
        const int64_t b0 = (int64_t)urank[u0] * w + base[u0];
        for (int jl = 0; jl < nn; jl++) {
          const int j = j0 + jl, g = h.ua + j;
          pos[g] = b0 + nj + jl;
          for (int c = 0; c < 3; c++) { pos[N + 3 * g + c] = b0 + nj + nn + 3 * jl + c; pos[4 * N + 3 * g + c] = b0 + nj + 4 * nn + 3 * jl + c; }
          for (int c = 0; c < 4; c++) pos[7 * N + 4 * g + c] = b0 + nj + 7 * nn + 4 * jl + c;
          for (int sl = 0; sl < h.K; sl++) {
            const int part = (h.air && sl >= 6 && sl < 15) ? 1 + (sl - 6) / 3 : 0;
            const int u = u0 + part;
            const int local = part ? sl - (6 + 3 * (part - 1)) : (sl >= 6 ? sl - skip : sl);
            pos[(size_t)11 * N + compact_index(h, sl, j)] = (int64_t)urank[u] * w + base[u] + (int64_t)local * nn + jl;
          }
        }
        if (j0 == 0) pos[(size_t)11 * N + h.voff + (int64_t)h.K * h.n] = b0 + (int64_t)(h.K - skip) * nn;
      }
  }
  for (int64_t v : pos)
    if (v < 0) return fail(GEL_ERR_ARG, "shard plan: an output entry without an owner (internal)");
  // the device copies first: a failure leaves the previous plan in place, on the host and on the device
  DeviceArray<int64_t> d_base, d_pos;
  if (p->device != GEL_DEVICE_NONE) {
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(d_base.upload(base)); HIPCHK(d_pos.upload(pos));
    HIPCHK(drain(p));   // launches in flight, on the handle's stream or on the caller's, still read the old plan
  }
  p->d_unit_base = std::move(d_base);
  p->d_shard_pos = std::move(d_pos);
  p->shard_begin.assign(unit_begin, unit_begin + nranks + 1);
  p->unit_base = base;
  p->shard_width = w;
  *width = w;
  if (res_pos) std::memcpy(res_pos, pos.data(), sizeof(int64_t) * 11 * (size_t)N);
  if (jvar_pos) std::memcpy(jvar_pos, pos.data() + (size_t)11 * N, sizeof(int64_t) * (size_t)V);
  return GEL_OK;
}

// The plan is state of the handle and the next gel_shard_plan call replaces it, so the caller states the plan its buffer was sized
// for (nranks, width): a buffer allocated as [old nranks][B][old width] must never be written with the new plan's offsets.
static int check_plan(const gel_problem* p, int32_t nranks, int64_t width) {
  if (p->shard_width <= 0) return fail(GEL_ERR_ARG, "gel_shard_plan has not been called on this handle");
  if (nranks != (int32_t)p->shard_begin.size() - 1 || width != p->shard_width)
    return fail(GEL_ERR_ARG, "the handle's shard plan is not the one this buffer was sized for (gel_shard_plan was called again: plan once more, or use one handle per plan)");
  return GEL_OK;
}

int gel_eval_shard_packed_device(gel_problem* p, int32_t B, const double* d_x, double* d_out, int32_t rank, int32_t nranks_expected,
                                 int64_t width_expected, void* stream) {
  if (!p || !d_x || !d_out || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NO_EXACT(p, "gel_eval_shard_packed_device");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (int rc = check_plan(p, nranks_expected, width_expected)) return rc;
  if (!p->d_unit_base.get()) return fail(GEL_ERR_ARG, "gel_shard_plan has not been called on this handle");
  const int nranks = (int)p->shard_begin.size() - 1;
  if (rank < 0 || rank >= nranks) return fail(GEL_ERR_ARG, "rank outside the plan");
  const int32_t u0 = p->shard_begin[rank], cnt = p->shard_begin[rank + 1] - u0;
  if (cnt == 0) return GEL_OK;
  gel::ProblemDev dv = p->dev;
  dv.chunks = p->d_chunks.get();  // unit ids refer to the phase-ordered list
  dv.chunk0 = 0;
  dv.unit0 = u0;
  dv.nunits = cnt;
  dv.shard_width = p->shard_width;
  dv.unit_base = p->d_unit_base.get();
  double* slice = d_out + (size_t)rank * (size_t)B * (size_t)p->shard_width;
  HIPCHK(gel::launch_eval(dv, B, d_x, slice, slice, stream_of(p, stream)));
  return GEL_OK;
}

int gel_shard_unpack_device(gel_problem* p, int32_t B, const double* d_out, double* d_res, double* d_jvar, int32_t nranks_expected,
                            int64_t width_expected, void* stream) {
  if (!p || !d_out || B < 1 || (!d_res && !d_jvar)) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  if (int rc = check_plan(p, nranks_expected, width_expected)) return rc;
  if (!p->d_shard_pos.get()) return fail(GEL_ERR_ARG, "gel_shard_plan has not been called on this handle");
  HIPCHK(gel::launch_shard_unpack(11 * p->dims.N, p->dims.num_var_entries, p->shard_width, B, p->d_shard_pos.get(), d_out, d_res, d_jvar,
                                  stream_of(p, stream)));
  return GEL_OK;
}

int gel_fill_full_device(gel_problem* p, int32_t B, double* d_jfull, void* stream) {
  if (!p || !d_jfull || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(gel::launch_fill_full(p->dims.total_nnz, B, p->d_cval.get(), d_jfull, stream_of(p, stream)));
  return GEL_OK;
}

int gel_update_full_device(gel_problem* p, int32_t B, const double* d_jvar, double* d_jfull, void* stream) {
  if (!p || !d_jvar || !d_jfull || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(gel::launch_update_full(p->dims.total_nnz, p->dims.num_var_entries, p->nvar_entries, B, p->d_vdst.get(), p->d_vsrc.get(),
                                 p->nvar_lines, p->d_vline.get(), p->d_src.get(), p->d_cval.get(), d_jvar, d_jfull,
                                 stream_of(p, stream)));
  return GEL_OK;
}

int gel_eval_full_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, double* d_jfull, void* stream) {
  if (!p || !d_x || !d_jvar || !d_jfull || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  hipStream_t s = stream_of(p, stream);
  gel::ProblemDev dv = p->dev;
  dv.cached_out = 1;   // the compact values are read again by the update below: kept in the caches when the launch fits them
  HIPCHK(launch_defects(p, dv, B, d_x, d_res, d_jvar, s));
  HIPCHK(gel::launch_update_full(p->dims.total_nnz, p->dims.num_var_entries, p->nvar_entries, B, p->d_vdst.get(), p->d_vsrc.get(),
                                 p->nvar_lines, p->d_vline.get(), p->d_src.get(), p->d_cval.get(), d_jvar, d_jfull, s));
  return GEL_OK;
}

int gel_expand_full_device(gel_problem* p, int32_t B, const double* d_jvar, double* d_jfull, void* stream) {
  if (!p || !d_jvar || !d_jfull || B < 1) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(gel::launch_expand(p->dims.total_nnz, p->dims.num_var_entries, B, p->d_cval.get(), p->d_src.get(), d_jvar, d_jfull,
                            stream_of(p, stream)));
  return GEL_OK;
}

int gel_sync(gel_problem* p, void* stream) {
  if (!p) return fail(GEL_ERR_ARG, "null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  hipStream_t s = stream_of(p, stream);
  HIPCHK(hipMemcpyAsync(p->h_flag.get(), p->d_flag.get(), 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int rc = GEL_OK;
  if (*p->h_flag.get()) {
    HIPCHK(clear_flag(p, s));
    *p->h_flag.get() = 0;
    rc = GEL_NONFINITE;
  }
  if (s == p->caller_stream) p->caller_stream = nullptr;   // drained: the caller may destroy it now
  return rc;
}

// ------------- post-processing table (output_result.py:37-263) -------------
int gel_output_table(gel_problem* p, const double* x, const double* tx_res, double launch_lat_deg, double launch_lon_deg,
                     double* out) {
  if (!p || !x || !tx_res || !out) return fail(GEL_ERR_ARG, "null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  const int M = p->dims.M;
  // the section of every state node (output_result.py:121-143: section s owns its n + 1 state nodes)
  std::vector<int32_t> sec((size_t)M);
  for (size_t i = 0; i < p->ph.size(); i++)
    for (int k = 0; k <= p->ph[i].n; k++) sec[(size_t)p->ph[i].xa + k] = (int32_t)i;
  const size_t nx = (size_t)p->dims.num_vars, no = (size_t)M * gel::kOutputColumns;
  return staged_call(p, kStagedNoFlag, {staged_in(x, nx), staged_in(tx_res, (size_t)M), staged_in(sec.data(), (size_t)M), staged_out(out, no)},
                     [&](const gel::ProblemDev&, double* const* a) -> int {
                       HIPCHK(gel::launch_output(p->dev, M, a[0], a[1], reinterpret_cast<const int32_t*>(a[2]), launch_lat_deg, launch_lon_deg,
                                                 a[3], p->stream.get()));
                       return GEL_OK;
                     });
}

// ------------- from-file initial guess on the host (initialize.py:322-409) -------------
int gel_initial_guess(const gel_problem* p, int32_t nref, const double* t_ref, const double* table,
                      const double* knot_times, double* x) {
  if (!p || !t_ref || !table || !knot_times || !x || nref < 2) return fail(GEL_ERR_ARG, "bad argument (>= 2 reference rows)");
  // repeated times are legal (the example's table repeats every knot: end of one section = start of the next); a
  // bracket [lo, hi] found by lower_bound never has zero width unless the table STARTS with a repeat
  for (int k = 1; k < nref; k++)
    if (!(t_ref[k] >= t_ref[k - 1])) return fail(GEL_ERR_ARG, "reference times must not decrease");
  const int S = p->dims.S, M = p->dims.M, N = p->dims.N;
  // scipy interp1d(kind="linear", fill_value="extrapolate"): hi = first knot >= t clipped to [1, nref - 1], lo = hi - 1,
  // y = slope * (t - t_lo) + y_lo with slope = (y_hi - y_lo) / (t_hi - t_lo): the end intervals extend beyond the table
  auto interp = [&](double t, int col0, int ncol, double unit, double* out) {
    int hi = (int)(std::lower_bound(t_ref, t_ref + nref, t) - t_ref);
    hi = std::min(std::max(hi, 1), nref - 1);
    const int lo = hi - 1;
    for (int c = 0; c < ncol; c++) {
      const double ylo = table[(size_t)lo * 13 + col0 + c], yhi = table[(size_t)hi * 13 + col0 + c];
      const double slope = (yhi - ylo) / (t_ref[hi] - t_ref[lo]);
      const double rise = slope * (t - t_ref[lo]);  // its own statement: no fused multiply-add, the bits scipy produces
      out[c] = (rise + ylo) / unit;
    }
  };
  double* xm = x; double* xr = x + M; double* xv = x + 4 * (size_t)M; double* xq = x + 7 * (size_t)M;
  double* xu = x + 11 * (size_t)M; double* xt = x + 11 * (size_t)M + 2 * (size_t)N;
  for (int i = 0; i < S; i++) {
    const HostPhase& h = p->ph[i];
    const double to = knot_times[i], tf = knot_times[i + 1];
    for (int k = 0; k <= h.n; k++) {  // state nodes: tau_x = [-1, tau]
      const double tau = (k == 0) ? -1.0 : h.tau[k - 1];
      const double t = tau * (tf - to) / 2.0 + (tf + to) / 2.0;
      const int node = h.xa + k;
      interp(t, 0, 1, p->um, xm + node);
      interp(t, 1, 3, p->up, xr + 3 * (size_t)node);
      interp(t, 4, 3, p->uv, xv + 3 * (size_t)node);
      interp(t, 7, 4, 1.0, xq + 4 * (size_t)node);
    }
    for (int k = 0; k < h.n; k++) {   // control nodes: tau
      const double t = h.tau[k] * (tf - to) / 2.0 + (tf + to) / 2.0;
      interp(t, 11, 2, p->uu, xu + 2 * (size_t)(h.ua + k));
    }
  }
  for (int i = 0; i <= S; i++) xt[i] = knot_times[i] / p->ut;
  // a node time beyond a reference table that ends (or starts) with a repeated time extrapolates over a zero-width interval
  // (scipy does the same and returns NaN / Inf silently): report it
  for (int64_t i = 0; i < p->dims.num_vars; i++)
    if (!std::isfinite(x[i])) return GEL_NONFINITE;
  return GEL_OK;
}

// ------------- one callback = one device round trip -------------
int gel_eval_callback(gel_problem* p, const double* x, const gel_callback_io* io) {
  if (!p || !x || !io) return fail(GEL_ERR_ARG, "null argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  int rc = ensure_capacity(p, 1);
  if (rc) return rc;
  const size_t nlin = p->lin_rows.size(), nfn = p->fn_rows.size(), R = nlin + nfn;
  const bool rows = io->rows_con && R;
  size_t off_c[3], off_j[3], atotal = 0;
  bool aero = false;
  for (int k = 0; k < 3; k++) {
    const size_t n = p->aero.rows[k].size();
    off_c[k] = atotal; atotal += (io->aero_con[k] && n) ? n : 0;
    off_j[k] = atotal; atotal += (io->aero_con[k] && n && io->aero_jac[k]) ? aero_jac_len(p, k) : 0;
    aero = aero || (io->aero_con[k] && n);
  }
  // the pinned outputs of the row table (con | jfn) and of the aero kinds behind them: the handle's pinned arena, as in the
  // host-buffer forms -- this call, too, runs on the handle's stream and returns synchronised
  const size_t nrows_out = rows ? R + 7 * nfn : 0;
  if (rows || aero) HIPCHK(p->h_arena.reserve(nrows_out + atotal));
  double* const h_rows = p->h_arena.get();
  double* const h_aero = h_rows + nrows_out;
  const bool x_pinned = p->cb_x[0].get() && (x == p->cb_x[0].get() || x == p->cb_x[1].get());
  if (!x_pinned) std::memcpy(p->h_x.get(), x, (size_t)p->dims.num_vars * 8);
  const double* const xin = x_pinned ? x : p->h_x.get();
  // everything reads x from and writes to pinned host memory: no copy commands
  gel::ProblemDev dv = p->dev;
  dv.flag = p->h_flag.get();
  const bool want_jac = io->vals_full != nullptr;
  const bool fused = io->res || want_jac;
  // GEL_CB_MODE=3 (measurement switch): the three launches of rounds 1-2, back to back on the handle's stream (compact path)
  static const int cb_mode = [] { const char* e = getenv("GEL_CB_MODE"); return e ? atoi(e) : 0; }();
  // exact handle with derivatives: the defect part is split out of the one-launch form -- the residual-only launch and the exact
  // kernel (launch_defects), then the row table and the aero kinds in launches of their own -- so that no forward-difference
  // sweep of the defect groups runs (nor flags a value that is then replaced)
  const bool split_exact = p->exact && want_jac;
  // likewise on a GEL_FLAG_EXACT_AERO_JAC handle whose aero gradients are asked for: the values-only aero launch and the exact aero
  // kernel (launch_aero_kinds) after the defect groups and the row table
  bool aero_jac = false;
  for (int k = 0; k < 3; k++) aero_jac = aero_jac || (io->aero_con[k] && io->aero_jac[k] && !p->aero.rows[k].empty());
  const bool split_aero = p->exact_aero && aero_jac;
  // and on a GEL_FLAG_EXACT_ROWS_JAC handle whose row jfn is asked for: rows_kernel for the values, then the exact row kernel
  // (launch_rows_kinds) -- no forward-difference sweep of the rows runs
  const bool split_rows = p->exact_rows && rows && io->rows_jfn;
  const bool coo = want_jac && cb_mode != 3 && !p->exact && !split_aero && !split_rows && coo_direct(p);
  if (coo) {
    if ((rc = ensure_full(p))) return rc;
    dv.coo_full = p->h_full.get(); dv.coo = p->d_coo.get();
  }
  dv.split_vel = 1;   // a whole evaluation: every part of every work item is in this launch
  const bool own_res = io->res && p->cb_res.get() && io->res == p->cb_res.get();
  double* const res_to = own_res ? p->cb_res.get() : p->h_res.get();
  gel::AeroLaunchOut out;
  if (aero)
    for (int k = 0; k < 3; k++) {
      const size_t n = p->aero.rows[k].size();
      out.nrows[k] = (int32_t)n;
      out.con[k] = (io->aero_con[k] && n) ? h_aero + off_c[k] : nullptr;
      out.jac[k] = (out.con[k] && io->aero_jac[k]) ? h_aero + off_j[k] : nullptr;
    }
  if (cb_mode == 3 || !fused || split_exact || split_aero || split_rows) {
    if (fused) HIPCHK(launch_defects(p, dv, 1, xin, res_to, want_jac ? p->h_jv.get() : nullptr, p->stream.get()));
    if (rows) HIPCHK(launch_rows_kinds(p, dv, 1, xin, h_rows, io->rows_jfn ? h_rows + R : nullptr, p->stream.get()));
    if (aero) HIPCHK(launch_aero_kinds(p, dv, (int)p->aero.nodes.size(), p->aero.d_nodes.get(), 1, xin, out, p->stream.get()));
  } else {
    // ONE launch: defect groups, aero kinds and row table as workgroup ranges of one grid (gel_kernels.hip callback_kernel)
    arm_done(p, dv);
    HIPCHK(gel::launch_callback(dv, want_jac, xin, res_to, want_jac ? p->h_jv.get() : nullptr,
                                aero ? (int)p->aero.nodes.size() : 0, p->aero.d_nodes.get(), aero ? &out : nullptr,
                                (int)nlin, p->d_lin_rows.get(), (int)nfn, p->d_fn_rows.get(), rows ? h_rows : nullptr,
                                (rows && io->rows_jfn) ? h_rows + R : nullptr, p->stream.get()));
  }
  HIPCHK(wait_done(p, dv));   // the ONE wait of the callback: the kernel's own word where it signals, else the runtime's synchronise
  if (io->res && !own_res) std::memcpy(io->res, p->h_res.get(), (size_t)11 * p->dims.N * 8);
  if (want_jac) {
    if (coo) finish_full(p, io->vals_full, io->fill_constants);
    else scatter_full(p, p->h_jv.get(), io->vals_full, io->fill_constants);
  }
  if (rows) {
    std::memcpy(io->rows_con, h_rows, R * 8);
    if (io->rows_jfn) std::memcpy(io->rows_jfn, h_rows + R, 7 * nfn * 8);
  }
  if (aero)
    for (int k = 0; k < 3; k++) {
      if (out.con[k]) std::memcpy(io->aero_con[k], out.con[k], p->aero.rows[k].size() * 8);
      if (out.jac[k]) std::memcpy(io->aero_jac[k], out.jac[k], aero_jac_len(p, k) * 8);
    }
  if (*p->h_flag.get()) { *p->h_flag.get() = 0; return GEL_NONFINITE; }
  return GEL_OK;
}

int gel_table_limits(int32_t wind_rows, int32_t ca_rows, int32_t n, int64_t* info) {
  if (wind_rows < 2 || ca_rows < 2 || !info) return fail(GEL_ERR_ARG, "bad argument");
  const size_t T = gel::staged_table_doubles(wind_rows, ca_rows), Tp = gel::padded_table_doubles(wind_rows, ca_rows);
  info[0] = (int64_t)T;
  info[1] = (int64_t)lds_room(gel::eval_lds_bytes_max(wind_rows, ca_rows) / 8 - Tp, true);
  info[2] = (int64_t)lds_room(gel::aero_lds_bytes(wind_rows, ca_rows) / 8 - Tp, true);
  info[3] = (n >= 2 && n < gel::kMeshMaxThreads) ? (int64_t)lds_room(gel::mesh_vector_doubles(n), true) : -1;
  info[4] = (int64_t)lds_room(gel::table_lds_bytes(wind_rows, ca_rows) / 8 - T, false);
  info[5] = (int64_t)gel::kLaunchMaxLds;
  info[6] = info[3] < 0 ? -1 : (int64_t)gel::mesh_vectors_per_group(wind_rows, ca_rows, n);
  return GEL_OK;
}

int gel_point_eval(int32_t kind, int32_t n, const double* in, const double* aux, int32_t aux_rows, double* out) {
  static const int nin[17] = {1, 3, 3, 6, 7, 1, 1, 2, 2, 8, 8, 8, 7, 4, 1, 5, 5}, nout[17] = {5, 3, 3, 3, 3, 3, 1, 4, 6, 8, 16, 4, 3, 7, 2, 18, 54};
  if (kind < 0 || kind > 16 || n < 0 || !in || !out) return fail(GEL_ERR_ARG, "bad argument");
  if (n == 0) return GEL_OK;
  const bool tabulated = kind == 5 || kind == 6 || kind == 9 || kind == 10 || kind == 15 || kind == 16;
  int rc = tabulated ? check_launch_lds("gel_point_eval", gel::point_lds_bytes(aux_rows), 5 * (size_t)std::max(aux_rows, 0), 5 * (size_t)std::max(aux_rows, 0), false) : GEL_OK;
  if (rc) return rc;
  rc = need_device();
  if (rc) return rc;
  double atm[gel::kAtmTableDoubles];
  size_t naux = 0;
  const double* hax = aux;
  std::vector<double> ext;  // kinds 5 / 6 / 9 / 10: the table rows followed by their per-interval slopes; kinds 15 / 16: the atmosphere table before them
  if (kind == 0) { gel::fill_atmosphere_table(atm); hax = atm; naux = gel::kAtmTableDoubles; aux_rows = 0; }
  else if (kind == 2) { if (!aux) return fail(GEL_ERR_ARG, "kind 2 needs aux[0] = barC20"); naux = 1; aux_rows = 0; }
  else if (tabulated) {
    const int w = (kind == 5 || kind == 10 || kind == 15 || kind == 16) ? 3 : 2;
    if (!aux || aux_rows < 2) return fail(GEL_ERR_ARG, "kinds 5, 6, 9, 10, 15 and 16 need a table of at least two rows");
    if (kind == 15 || kind == 16) { gel::fill_atmosphere_table(atm); ext.assign(atm, atm + gel::kAtmTableDoubles); }   // atmosphere | wind rows | slopes
    for (int k = 1; k < aux_rows; k++)
      if (!(aux[(size_t)w * k] > aux[(size_t)w * (k - 1)])) return fail(GEL_ERR_ARG, "table abscissae must increase strictly");
    std::vector<double> slopes;
    gel::append_rows_and_slopes(ext, slopes, aux, aux_rows, w);
    ext.insert(ext.end(), slopes.begin(), slopes.end());
    hax = ext.data(); naux = ext.size();
  }
  else { aux_rows = 0; }
  DeviceArray<double> i, a, o;
  HIPCHK(i.upload(in, (size_t)n * nin[kind])); HIPCHK(a.upload(hax, naux)); HIPCHK(o.reserve((size_t)n * nout[kind]));
  HIPCHK(gel::launch_point(kind, n, i.get(), a.get(), aux_rows, o.get(), nullptr));
  HIPCHK(hipMemcpy(out, o.get(), (size_t)n * nout[kind] * 8, hipMemcpyDeviceToHost));
  return GEL_OK;
}

}  // extern "C"
