// gel_host.hip -- host side of the engine: fixed sparsity pattern, device-resident problem, and the C-ABI of
// include/gelato_amd.h.  The extended-precision generators (LGR nodes, D, the mesh estimate's matrices) are gel_host_lgr.hip;
// what the host files share is gel_host_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gelato_amd.h"
#include "gel_device.h"
#include "gel_launch.h"
#include "gel_mesh.h"
#include "gel_jprod.h"
#include "gel_conprod.h"
#include "gel_interp.h"
#include "gel_prop.h"
#include "gel_proptan.h"
#include "gel_propadj.h"
#include "gel_outbatch.h"
#include "gel_quant.h"
#include "gel_comom.h"
#include "gel_host_internal.h"

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

namespace {

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(GEL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

// The only owners of device and pinned memory in this file: an array frees its block in its destructor (and when it is
// moved onto).  reserve() only grows: the old block goes first, and a failed allocation leaves the array empty with
// capacity 0 -- never a stale pointer.  upload() sizes the array for at least one element and copies the host data in.
template <class T, bool Pinned>
class HipArray {
 public:
  HipArray() = default;
  HipArray(HipArray&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  HipArray& operator=(HipArray&& o) noexcept {
    if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); }
    return *this;
  }
  ~HipArray() { reset(); }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  hipError_t reserve(size_t n) {
    if (cap_ >= n) return hipSuccess;
    reset();
    void* q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T)) : hipMalloc(&q, n * sizeof(T));
    if (e == hipSuccess) { p_ = static_cast<T*>(q); cap_ = n; }
    return e;
  }
  hipError_t upload(const T* h, size_t n) {
    if (const hipError_t e = reserve(std::max<size_t>(1, n))) return e;
    if (!n) return hipSuccess;
    if (Pinned) { std::memcpy(p_, h, n * sizeof(T)); return hipSuccess; }
    return hipMemcpy(p_, h, n * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t upload(const std::vector<T>& h) { return upload(h.data(), h.size()); }

 private:
  void reset() {
    if (p_) (void)(Pinned ? hipHostFree((void*)p_) : hipFree((void*)p_));
    p_ = nullptr;
    cap_ = 0;
  }
  T* p_ = nullptr;
  size_t cap_ = 0;  // elements
};
template <class T> using DeviceArray = HipArray<T, false>;
template <class T> using PinnedArray = HipArray<T, true>;

// A stream, created on demand; its destructor lets the work on it finish, then destroys it.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
  ~Stream() { if (s_) { hipStreamSynchronize(s_); hipStreamDestroy(s_); } }
  hipStream_t get() const { return s_; }
  hipError_t create() { return s_ ? hipSuccess : hipStreamCreate(&s_); }

 private:
  hipStream_t s_ = nullptr;
};

// doubles of one phase's block in the host table: sigma | Lx | Lu | I
inline size_t mesh_block_doubles(int n) { return (size_t)(n + 1) * (1 + (n + 1) + n + (n + 1)); }

// ---------------------------------------------------------------------------
struct HostPhase {
  int n, ua, xa;
  int air, air_fd, t_fd, q_fd, engine_on, hold;
  int K, s_vv, s_vq, s_vt, s_qq;
  int64_t voff;
  double thrust, massflow, area, nozzle;
  std::vector<double> D, tau;
};

}  // namespace

struct gel_problem {
  int device = 0;
  bool fd_recompute = false;   // GEL_FLAG_FD_RECOMPUTE (or a step too long for the difference form): the reference's recomputing sweeps
  bool exact = false;          // GEL_FLAG_EXACT_DEFECT_JAC: defect Jacobians by gel_kernels_exact.hip (residuals by the residual-only form)
  bool exact_aero = false;     // GEL_FLAG_EXACT_AERO_JAC: aero gradients by gel_kernels_exact_aero.hip (values by the values-only aero launch)
  bool exact_rows = false;     // GEL_FLAG_EXACT_ROWS_JAC: node-function rows' jfn by gel_kernels_exact_rows.hip (values by rows_kernel)
  bool aero_fused = true;      // GEL_AERO_FUSED (read when the handle is created): 0 = gel_eval_batch_aero_device by the two kernels
  Stream stream;
  // The last caller-owned stream a device-form entry point was given (stream_of); gel_sync on it clears it again.  Whatever releases
  // or replaces device memory that a device-form launch reads waits for this stream as well as for the handle's own (drain).
  hipStream_t caller_stream = nullptr;
  gel::ProblemDev dev{};
  std::vector<HostPhase> ph;
  gel_dims dims{};
  int64_t block_off[GEL_NUM_BLOCKS + 1]{};
  double um, up, uv, uu, ut, dx, barC20;
  // host copies of the pattern-derived data
  std::vector<double> cval;      // [total_nnz] constants (x-dependent entries 0)
  std::vector<int32_t> src;      // [total_nnz] gather map: -1 constant; s >= 0: compact[s]; s <= -2: -compact[-2 - s]
  std::vector<int64_t> var_idx;  // [V] compact slot -> the first full index that takes it with a plus sign
  struct Run { int64_t dst0, dstride, src0, sstride, len; double sign; };
  std::vector<Run> var_runs;     // the gather map as constant-stride runs (about one per (phase, slot, use): the n nodes)
  std::vector<int32_t> chunk_phase;  // [nchunks] phase of every 64-node work item
  // packed unit-shard exchange (gel_shard_plan): contiguous unit ranges per rank; every unit's entries of a vector form one
  // block at unit_base[unit] inside its rank's slice; shard_pos = the map back to the ordinary layouts
  std::vector<int32_t> shard_begin;  // [nranks + 1]
  std::vector<int64_t> unit_base;    // [4 * nchunks]
  int64_t shard_width = 0;
  DeviceArray<int64_t> d_unit_base;
  DeviceArray<int64_t> d_shard_pos;  // [11N + V]: rank * width + offset of every res entry, then of every compact value
  // aero path constraints, host tables and their device copies: gel_aero_configure builds a whole new set and
  // swaps it in, so a call that fails leaves the previous one in place
  struct Aero {
    std::vector<gel::AeroRowDev> rows[3];                   // kind 0 = AOA_max, 1 = dynamic_pressure_max, 2 = Q_alpha_max
    std::vector<gel::AeroNodeDev> nodes;                    // the constrained state nodes, shared by the kinds
    // gel_eval_batch_aero_device (defect groups + aero rows, one output record per vector): the record's layout, the per-phase
    // records of the rows the fused kernel's lanes write, and the constrained nodes they do not reach (state node 0 of a phase,
    // phases without aerodynamics) -- left to aero_wide_kernel
    int64_t ld = 0, off_con[2][3] = {{0, 0, 0}, {0, 0, 0}}, off_jac[2][3] = {{0, 0, 0}, {0, 0, 0}};
    std::vector<gel::AeroRowDev> part_rows[2][3];           // the rows of part A (the lanes') and part B (the rest), per kind
    std::vector<int32_t> part_of[3];                        // per row of a kind: part | (row inside the part) << 1
    std::vector<int64_t> partA_base[3];                     // per row of part A: first double of its spec's block in the record
    int64_t partA_len = 0;                                  // doubles of part A (part B's sections follow)
    int64_t dump = 0;                                       // first double of the dump area at the end of part A
    std::vector<gel::AeroNodeDev> part_nodes[2];
    std::vector<gel::AeroPhaseDev> ph;
    DeviceArray<gel::AeroNodeDev> d_nodes, d_part_nodes[2];
    DeviceArray<gel::AeroPhaseDev> d_ph;
  } aero;
  // device buffers (static)
  DeviceArray<gel::PhaseDev> d_phases;
  DeviceArray<int32_t> d_node_phase;
  DeviceArray<int4> d_chunks;         // work items in phase order (what gel_chunk_phase / shard ranges index)
  DeviceArray<int4> d_chunks_sorted;  // the same items, dearest phase type first (whole launches)
  DeviceArray<double> d_Dsw;          // D per work item in the feed order of v_mfma_f64_16x16x4_f64
  DeviceArray<double> d_Dst;          // the same, row-tile major (one wavefront per row tile)
  DeviceArray<double> d_Dt, d_tau, d_tables, d_cval;
  DeviceArray<int32_t> d_src;
  DeviceArray<int32_t> d_vdst, d_vsrc;   // the x-dependent entries of the gather map: destination (ascending), signed source
  int32_t nvar_entries = 0;
  DeviceArray<int32_t> d_vline;   // the 64-byte lines (index / 8) of a value vector that hold an x-dependent entry
  int32_t nvar_lines = 0;
  // COO-direct output of the one-vector latency path (gel_eval_kernel.h "COO-DIRECT"): first entry of the eight groups of runs per
  // phase; the runs of the gather map that are left to the host (dense velocity / quaternion blocks); the engine's own full value
  // array in pinned host memory (constants laid down once; the kernel and the host scatter rewrite the x-dependent entries)
  std::vector<int32_t> coo_tab;   // [8 * S]; empty: the mode is not available for this problem
  std::vector<Run> rest_runs;
  DeviceArray<int32_t> d_coo;
  PinnedArray<double> h_full;
  PinnedArray<double> cb_res;     // pinned residual vector a caller may name as its own output (gel_pinned_buffers): no copy then
  PinnedArray<double> cb_x[2];    // two pinned decision-vector buffers a caller may fill in turn and pass as x: read in place
  DeviceArray<int32_t> d_flag;
  // B = 1 / small-batch working set
  int capB = 0;
  DeviceArray<double> d_x, d_res, d_jv;
  PinnedArray<double> h_x, h_res, h_jv;
  PinnedArray<int32_t> h_flag;
  // The working set of every synchronous host-buffer call of the handle and of the plans that refer to it (staged_call): those calls
  // run on the handle's stream and return synchronised, so no two of them are in flight together and one pair serves them all.
  // Both only grow and are kept until the handle is closed.
  DeviceArray<double> d_arena;
  PinnedArray<double> h_arena;
  // the envelope partials of gel_output_table_batch* (DESIGN.md 3.16): the device form's buffers are the caller's, so the partials
  // cannot live beside them in the arena; only grows, after a drain
  DeviceArray<double> d_outws;
  // the workspace of gel_batch_quantiles* (gel_quant.h quant_layout), capped at gel::kQuantWsCap: only grows, after a
  // drain.  quant_targets: the (column, rank) pairs of the last call, for gel_batch_quantiles_last
  DeviceArray<char> d_quantws;
  int64_t quant_targets = 0;
  // the workspace of gel_batch_comoments* (gel_comom.h com_layout), capped at gel::kComWsCap: only grows, after a drain
  DeviceArray<char> d_comws;
  // gel_jac_fd working set: kept between calls; the residuals of all num_vars + 1 perturbed vectors are
  // re-used while x stays the same (the four groups are asked for one after the other)
  struct JacFd {
    DeviceArray<double> x, Xp, res, J;
    // every phase as its own one-phase problem (gel_jac_fd differences phase by phase)
    DeviceArray<gel::PhaseDev> d_subphases;                     // [S] the phase records with ua = xa = 0
    DeviceArray<int4> d_subchunks;                              // the phase-ordered work items with phase index 0
    DeviceArray<int32_t> d_colmap;                              // per phase: local column -> global column
    std::vector<int32_t> sub_chunk0, sub_nchunks, sub_col0;     // [S] first work item, work items, first colmap entry
    std::vector<size_t> sub_res0;                               // [S] first double of the phase's residuals in res
    std::vector<double> last_x;                                 // empty = nothing cached
    int status = GEL_OK;
  } jfd;
  struct Done {
    DeviceArray<int32_t> d_ctr;                                 // self-signalling one-vector launches (ProblemDev::done_flag): device counter,
    PinnedArray<volatile int32_t> h_word;                       // pinned host word, sequence number of the last armed launch
    int32_t seq = 0;
    long long ema_us = 100;                                     // running estimate of a self-signalling launch's wait (sets the spin budget)
  } done;
  // knot / terminal / user rows (gel_rows_configure)
  std::vector<gel::LinRowDev> lin_rows;
  std::vector<gel::FnRowDev> fn_rows;
  DeviceArray<gel::LinRowDev> d_lin_rows;
  DeviceArray<gel::FnRowDev> d_fn_rows;
  // collocation error estimate (gel_mesh_*): per phase the host block sigma | Lx | Lu | I (row-major) at hoff[i], the device
  // copy transposed (gel_mesh.h); none when a phase has more nodes than mesh_kernel's workgroup has lanes
  struct Mesh {
    std::vector<double> host;
    std::vector<size_t> hoff;
    std::vector<gel::MeshPhaseDev> ph;
    int32_t npts = 0;
    size_t lds_max = 0;     // LDS of the widest phase's workgroup (gel::mesh_lds_bytes), host-only handles included
    gel::MeshDev dev{};
    DeviceArray<double> d_mat;
    DeviceArray<gel::MeshPhaseDev> d_ph;
  } mesh;
  // Jacobian products from the compact values (gel_jac_*): the operator tables of gel_jprod.h, built from the
  // pattern walk (host-only handles included; the host product reads the same arrays), and their device copies
  struct Jprod {
    std::vector<int32_t> it;
    std::vector<double> dt;
    std::vector<gel::JprodPhaseDev> ph;
    int64_t info[4] = {0, 0, 0, 0};                           // non-zero constant entries, variable entries, longest row, longest column
    int threads = 512;                                        // lanes per workgroup (GEL_JPROD_THREADS = 256 when the handle is created: measurement switch)
    int32_t nin_max[2] = {0, 0};                              // largest local input count of a phase: J v, J^T lambda
    gel::JprodDev dev{};
    DeviceArray<int32_t> d_it;
    DeviceArray<double> d_dt;
    DeviceArray<gel::JprodPhaseDev> d_ph;
    DeviceArray<double> d_tpart;                              // [B][S][2] partial sums of the time columns of J^T lambda
  } jp;
  // Products with K, the Jacobian of every row that is not a defect row (gel_con_*): the operator tables of
  // gel_conprod.h in both directions (0: by row, K v; 1: by column, K^T lambda), rebuilt as a whole by gel_rows_configure and
  // gel_aero_configure and swapped in with the tables they come from (host-only handles included; the host product reads the
  // same arrays), and their device copies
  struct Conprod {
    int32_t nlin = 0, nfn = 0, nrows[3] = {0, 0, 0};
    int64_t R = 0, nnz = 0, max_row = 0, max_col = 0, jac_len[3] = {0, 0, 0};
    struct Dir {
      std::vector<int32_t> ptr, idx, src;
      std::vector<int64_t> offd, offr;                        // dense form, record form
      std::vector<double> cval;
      DeviceArray<int32_t> d_ptr, d_idx, d_src;
      DeviceArray<int64_t> d_offd, d_offr;
      DeviceArray<double> d_cval;
    } dir[2];
  } conprod;
  // large host batches (gel_eval_batch): two staging slots of kPipeEvals decision vectors each, every
  // slot with its own stream, so that PCIe in, kernel, PCIe out and the host copies of neighbouring
  // sub-batches overlap
  struct Slot {
    DeviceArray<double> d_x, d_res, d_jv;
    PinnedArray<double> h_x, h_res, h_jv;
    DeviceArray<int32_t> d_flag;
    PinnedArray<int32_t> h_flag;
    Stream stream;
    int64_t first = 0;  // sub-batch in flight: [first, first + count)
    int count = 0;
    bool res = false, jac = false;
  } slot[2];
  int pipe_evals = 0;  // capacity of a slot (0 = not allocated)

  // Nothing may still run on the handle's streams when its memory goes: the device is made current and every stream is
  // drained first; then the members free themselves.  A host-only handle owns no device resource and makes no HIP call.
  ~gel_problem() {
    if (device == GEL_DEVICE_NONE) return;
    hipSetDevice(device);
    for (hipStream_t s : {stream.get(), slot[0].stream.get(), slot[1].stream.get(), caller_stream})
      if (s) (void)hipStreamSynchronize(s);   // a caller's stream that is gone by now answers with an error: nothing runs on it
  }
};

namespace {

// kind: 0 = constant value; 1 = x-dependent, value = compact[slot]; 2 = x-dependent, value = -compact[slot]
// (slot = compact index within the eval; several entries may name the same slot)
using Visitor = std::function<void(int block, int64_t k, int32_t row, int32_t col, int kind, double cval, int64_t slot)>;

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

// global column of every local column of phase i as a one-phase problem: [mass n+1 | pos 3(n+1) | vel 3(n+1) | quat 4(n+1) | u 2n | t0 tf]
static void phase_columns(const gel_problem* p, int i, std::vector<int32_t>& colmap) {
  const HostPhase& h = p->ph[i];
  const int n = h.n, M = (int)p->dims.M, N = (int)p->dims.N;
  for (int k = 0; k <= n; k++) colmap.push_back(h.xa + k);                                  // mass
  for (int k = 0; k < 3 * (n + 1); k++) colmap.push_back(M + 3 * h.xa + k);                  // position
  for (int k = 0; k < 3 * (n + 1); k++) colmap.push_back(4 * M + 3 * h.xa + k);              // velocity
  for (int k = 0; k < 4 * (n + 1); k++) colmap.push_back(7 * M + 4 * h.xa + k);              // quaternion
  for (int k = 0; k < 2 * n; k++) colmap.push_back(11 * M + 2 * h.ua + k);                   // u
  colmap.push_back(11 * M + 2 * N + i); colmap.push_back(11 * M + 2 * N + i + 1);            // t0, tf
}

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

// A host-only handle is refused with the code and the text of the entry point's family.
#define NEED_DEVICE(p, code, text)                                  \
  do {                                                              \
    if ((p)->device == GEL_DEVICE_NONE) return fail(code, text);    \
  } while (0)
constexpr const char* kNoGpu = "host-only handle: nothing can be evaluated without a GPU (no CPU fallback)";
constexpr const char* kNoGpuInterp = "host-only handle: the device interpolation needs a GPU (gel_interp_host runs on the host)";
constexpr const char* kNoGpuJprod = "host-only handle: the device products need a GPU (gel_jac_products_host runs on the host)";
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
constexpr const char* kNoGpuConprod = "host-only handle: the device products need a GPU (gel_con_products_host runs on the host)";

// The defect groups of B vectors: one launch of the fused kernel; on a handle created with GEL_FLAG_EXACT_DEFECT_JAC, a call with
// derivatives is the residual-only launch of the fused kernel (when residuals are asked for) followed by the exact-Jacobian kernel.
hipError_t launch_defects(const gel_problem* p, const gel::ProblemDev& dv, int B, const double* x, double* res, double* jvar,
                          hipStream_t s) {
  if (!p->exact || !jvar) return gel::launch_eval(dv, B, x, res, jvar, s);
  if (res) {
    const hipError_t e = gel::launch_eval(dv, B, x, res, nullptr, s);
    if (e != hipSuccess) return e;
  }
  return gel::launch_eval_exact(dv, B, x, jvar, s);
}
// The aero kinds of B vectors (launch_aero's outputs and addressing); on a handle created with GEL_FLAG_EXACT_AERO_JAC, a call with
// gradients is the values-only aero launch followed by the exact aero kernel (same outputs: the constraint values bit-identical).
// wide: the records' part B (launch_aero_wide); ld / spec_major: the records of gel_eval_batch_aero_device.
hipError_t launch_aero_kinds(const gel_problem* p, const gel::ProblemDev& dv, int nnodes, const gel::AeroNodeDev* nodes, int B,
                             const double* x, const gel::AeroLaunchOut& out, hipStream_t s, long long ld = 0, bool spec_major = false,
                             bool wide = false) {
  const bool jac = out.jac[0] || out.jac[1] || out.jac[2];
  if (!p->exact_aero || !jac) return wide ? gel::launch_aero_wide(dv, nnodes, nodes, B, x, out, ld, s)
                                          : gel::launch_aero(dv, nnodes, nodes, B, x, out, s, ld, spec_major);
  gel::AeroLaunchOut vals = out;
  for (int k = 0; k < 3; k++) vals.jac[k] = nullptr;
  const hipError_t e = wide ? gel::launch_aero_wide(dv, nnodes, nodes, B, x, vals, ld, s)
                            : gel::launch_aero(dv, nnodes, nodes, B, x, vals, s, ld, spec_major);
  if (e != hipSuccess) return e;
  return gel::launch_aero_exact(dv, nnodes, nodes, B, x, out, s, ld, !wide && spec_major);
}
// The row table of B vectors (launch_rows' outputs); on a handle created with GEL_FLAG_EXACT_ROWS_JAC, a call with jfn is rows_kernel
// without the jfn output followed by the exact row kernel (the values bit-identical, no forward difference formed)
hipError_t launch_rows_kinds(const gel_problem* p, const gel::ProblemDev& dv, int B, const double* x, double* con, double* jfn,
                             hipStream_t s) {
  const int nlin = (int)p->lin_rows.size(), nfn = (int)p->fn_rows.size();
  if (!p->exact_rows || !jfn) return gel::launch_rows(dv, nlin, p->d_lin_rows.get(), nfn, p->d_fn_rows.get(), B, x, con, jfn, s);
  const hipError_t e = gel::launch_rows(dv, nlin, p->d_lin_rows.get(), nfn, p->d_fn_rows.get(), B, x, con, nullptr, s);
  if (e != hipSuccess) return e;
  return gel::launch_rows_exact(dv, nfn, p->d_fn_rows.get(), B, x, jfn, s);
}
#define NO_EXACT(p, what)                                                                                                   \
  do {                                                                                                                      \
    if ((p)->exact) return fail(GEL_ERR_ARG, what " has no exact-Jacobian form (handle created with GEL_FLAG_EXACT_DEFECT_JAC)"); \
  } while (0)

// calls moving less than this are served zero-copy out of the pinned staging buffers (run_host)
constexpr size_t kZeroCopyBytes = (size_t)1 << 20;

// ---- One synchronous host-buffer call on the handle's own stream (staged_call): every gel_* entry point that takes host arrays,
// runs a launch on them and returns synchronised, apart from the one-vector and pipelined evaluation paths (run_host*).
// A buffer of the call in the caller's memory: read before the launch (src), written after it (dst), or both.  One that the caller
// did not pass (NULL) takes no space and the launch sees nullptr; one of length 0 still has an address.
struct StagedBuf { const void* src; void* dst; size_t bytes; };
template <class T> StagedBuf staged_in(const T* h, size_t n) { return {h, nullptr, n * sizeof(T)}; }
template <class T> StagedBuf staged_out(T* h, size_t n) { return {nullptr, h, n * sizeof(T)}; }
template <class T> StagedBuf staged_inout(T* h, size_t n) { return {h, h, n * sizeof(T)}; }
enum { kStagedZeroCopy = 1,    // a call moving at most kZeroCopyBytes is served out of pinned host memory: no copy engine, one wait
       kStagedNoFlag = 2 };    // the non-finite flag is not read back
constexpr int kStagedMaxBufs = 8;

// Lays the buffers out in the handle's arena (each at a multiple of 256 bytes, hipMalloc's own alignment), brings the inputs in,
// runs launch(dv, a) -- a[i] the address of buffer i, dv the handle's ProblemDev with the flag word of the branch; returns a gel
// status -- on the handle's stream, brings the outputs out and waits.  Zero-copy branch: memcpy into the pinned arena, the kernel
// reads and writes it in place and raises h_flag, memcpy out.  Copied branch: hipMemcpyAsync into the device arena, outputs and
// d_flag back behind the launch.  GEL_NONFINITE resets the host word and, on the copied branch, the device's (clear_flag waits).
// Once something is enqueued every return is behind a hipStreamSynchronize: after an error no copy that names a caller's array
// is still pending.
template <class Launch>
int staged_call(gel_problem* p, int opts, std::initializer_list<StagedBuf> bufs, const Launch& launch) {
  if (bufs.size() > (size_t)kStagedMaxBufs) return fail(GEL_ERR_ARG, "staged_call: too many buffers");
  const StagedBuf* b = bufs.begin();
  const int n = (int)bufs.size();
  size_t off[kStagedMaxBufs], total = 0, moved = 0;
  for (int i = 0; i < n; i++) {
    off[i] = total;
    if (!b[i].src && !b[i].dst) continue;
    total += (std::max<size_t>(b[i].bytes, 1) + 255) / 256 * 256;
    moved += b[i].bytes;
  }
  const bool zero_copy = (opts & kStagedZeroCopy) && moved <= kZeroCopyBytes, flag = !(opts & kStagedNoFlag);
  hipStream_t s = p->stream.get();
  char* base;
  if (zero_copy) {
    HIPCHK(p->h_arena.reserve(total / 8));
    base = reinterpret_cast<char*>(p->h_arena.get());
  } else {
    if (p->d_arena.capacity() < total / 8) {
      HIPCHK(hipStreamSynchronize(s));   // a resident call of a plan, enqueued on this stream, may still be running: the old block goes
      HIPCHK(p->d_arena.reserve(total / 8));
    }
    base = reinterpret_cast<char*>(p->d_arena.get());
  }
  double* a[kStagedMaxBufs];
  for (int i = 0; i < n; i++) a[i] = (b[i].src || b[i].dst) ? reinterpret_cast<double*>(base + off[i]) : nullptr;
  gel::ProblemDev dv = p->dev;
  if (zero_copy) dv.flag = p->h_flag.get();
  const auto enqueue = [&]() -> int {
    for (int i = 0; i < n; i++) {
      if (!b[i].src || !b[i].bytes) continue;
      if (zero_copy) std::memcpy(a[i], b[i].src, b[i].bytes);
      else HIPCHK(hipMemcpyAsync(a[i], b[i].src, b[i].bytes, hipMemcpyHostToDevice, s));
    }
    if (const int rc = launch(dv, a)) return rc;
    if (zero_copy) return GEL_OK;
    for (int i = 0; i < n; i++)
      if (b[i].dst && b[i].bytes) HIPCHK(hipMemcpyAsync(b[i].dst, a[i], b[i].bytes, hipMemcpyDeviceToHost, s));
    if (flag) HIPCHK(hipMemcpyAsync(p->h_flag.get(), p->d_flag.get(), 4, hipMemcpyDeviceToHost, s));
    return GEL_OK;
  };
  if (const int rc = enqueue()) {
    (void)hipStreamSynchronize(s);   // the error of the step that failed is the one reported
    return rc;
  }
  HIPCHK(hipStreamSynchronize(s));
  if (zero_copy)
    for (int i = 0; i < n; i++)
      if (b[i].dst && b[i].bytes) std::memcpy(b[i].dst, a[i], b[i].bytes);
  if (flag && *p->h_flag.get()) {
    *p->h_flag.get() = 0;
    if (!zero_copy) HIPCHK(clear_flag(p, s));
    return GEL_NONFINITE;
  }
  return GEL_OK;
}

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

// ---- generic forward difference, phase by phase (lib/jac_fd.py:29-62 on the four defect residuals) ----
// working set: x, the perturbed local vectors of the LARGEST phase (reused phase after phase), the residuals of every phase's
// perturbed vectors (kept while x stays the same: the four groups are asked for one after the other)
static int jfd_allocate(gel_problem* p) {
  if (p->jfd.x.get()) return GEL_OK;
  const size_t nv = (size_t)p->dims.num_vars;
  size_t xp_max = 0, res_tot = 0;
  p->jfd.sub_res0.clear();
  for (int i = 0; i < p->dims.S; i++) {
    const size_t n = p->ph[i].n, nloc = 13 * n + 13;
    xp_max = std::max(xp_max, (nloc + 1) * nloc);
    p->jfd.sub_res0.push_back(res_tot);
    res_tot += (nloc + 1) * 11 * n;
  }
  DeviceArray<double> jx, jxp, jres;   // all or nothing: a later call must not find a partial set
  if (jx.reserve(nv) != hipSuccess || jxp.reserve(xp_max) != hipSuccess || jres.reserve(res_tot) != hipSuccess)
    return fail(GEL_ERR_ALLOC, "gel_jac_fd: device allocation failed");
  p->jfd.x = std::move(jx); p->jfd.Xp = std::move(jxp); p->jfd.res = std::move(jres);
  return GEL_OK;
}

// one residual evaluation per (phase, local column) of the vector at d_x: launches only
static int jfd_evaluate(gel_problem* p, const double* d_x, hipStream_t s) {
  for (int i = 0; i < p->dims.S; i++) {
    const int n = p->ph[i].n, nloc = 13 * n + 13;
    gel::ProblemDev dv = p->dev;   // the phase as a one-phase problem: same tables, D, tau; local index space
    dv.S = 1; dv.N = n; dv.M = n + 1; dv.nvars = nloc; dv.V = 0;
    dv.phases = p->jfd.d_subphases.get() + i;
    dv.chunks = p->jfd.d_subchunks.get() + p->jfd.sub_chunk0[i]; dv.nchunks = p->jfd.sub_nchunks[i]; dv.chunk0 = 0;
    HIPCHK(gel::launch_perturb_local(nloc, p->dx, d_x, p->jfd.d_colmap.get() + p->jfd.sub_col0[i], p->jfd.Xp.get(), s));
    HIPCHK(gel::launch_eval(dv, nloc + 1, p->jfd.Xp.get(), p->jfd.res.get() + p->jfd.sub_res0[i], nullptr, s));
  }
  return GEL_OK;
}

static inline int jfd_w(int group) { return (group == 0) ? 1 : (group == 3) ? 4 : 3; }   // rows per node of the group

// the group's quotients from the residuals of jfd_evaluate: dense [num_rows[group]][num_vars] (zeros, then every phase's block at its
// rows and mapped columns) or the blocks alone, one after the other, [w n_i][13 n_i + 13] each; -> doubles written
static int jfd_quotients(gel_problem* p, int group, int blocks, double* d_J, hipStream_t s, size_t* count) {
  const size_t nv = (size_t)p->dims.num_vars, nrows = (size_t)p->dims.num_rows[group];
  const int w = jfd_w(group);
  if (!blocks) HIPCHK(hipMemsetAsync(d_J, 0, nrows * nv * 8, s));
  size_t off = 0;
  for (int i = 0; i < p->dims.S; i++) {
    const int n = p->ph[i].n, nloc = 13 * n + 13;
    const int roff_loc = (group == 0) ? 0 : (group == 1) ? n : (group == 2) ? 4 * n : 7 * n;
    if (blocks)
      HIPCHK(gel::launch_quotient_local(nloc, 11 * n, roff_loc, w * n, p->dx, p->jfd.res.get() + p->jfd.sub_res0[i], d_J + off, (long long)nloc, 0,
                                        nullptr, s));
    else
      HIPCHK(gel::launch_quotient_local(nloc, 11 * n, roff_loc, w * n, p->dx, p->jfd.res.get() + p->jfd.sub_res0[i], d_J, (long long)nv,
                                        w * p->ph[i].ua, p->jfd.d_colmap.get() + p->jfd.sub_col0[i], s));
    off += (size_t)w * n * nloc;
  }
  *count = blocks ? off : nrows * nv;
  return GEL_OK;
}

static size_t jfd_block_doubles(const gel_problem* p, int group) {
  size_t tot = 0;
  for (int i = 0; i < p->dims.S; i++) tot += (size_t)jfd_w(group) * p->ph[i].n * (13 * (size_t)p->ph[i].n + 13);
  return tot;
}

static int jfd_host(gel_problem* p, int32_t group, const double* x, double* J, int blocks) {
  if (!p || !x || !J || group < 0 || group >= GEL_NUM_GROUPS) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  int rc = ensure_slots(p);  // the two pinned staging slots also carry J back to the caller
  if (rc) return rc;
  if ((rc = jfd_allocate(p))) return rc;
  const size_t nv = (size_t)p->dims.num_vars, nrows = (size_t)p->dims.num_rows[group];
  const size_t need = blocks ? jfd_block_doubles(p, group) : nrows * nv;
  HIPCHK(p->jfd.J.reserve(need));
  // the perturbed evaluations -- unless the same x was just differenced
  if (p->jfd.last_x.size() != nv || std::memcmp(p->jfd.last_x.data(), x, nv * 8) != 0) {
    p->jfd.last_x.clear();
    HIPCHK(hipMemcpyAsync(p->jfd.x.get(), x, nv * 8, hipMemcpyHostToDevice, p->stream.get()));
    if ((rc = jfd_evaluate(p, p->jfd.x.get(), p->stream.get()))) return rc;
    HIPCHK(hipMemcpyAsync(p->h_flag.get(), p->d_flag.get(), 4, hipMemcpyDeviceToHost, p->stream.get()));
    HIPCHK(hipStreamSynchronize(p->stream.get()));
    p->jfd.status = GEL_OK;
    if (*p->h_flag.get()) { *p->h_flag.get() = 0; HIPCHK(clear_flag(p, p->stream.get())); p->jfd.status = GEL_NONFINITE; }
    p->jfd.last_x.assign(x, x + nv);
  }
  size_t total = 0;
  if ((rc = jfd_quotients(p, group, blocks, p->jfd.J.get(), p->stream.get(), &total))) return rc;
  HIPCHK(hipStreamSynchronize(p->stream.get()));
  // J -> caller through the two pinned slots: D2H of piece i+1 overlaps the host copy of piece i
  const size_t piece = (size_t)p->pipe_evals * (size_t)std::max<int64_t>(p->dims.num_var_entries, 1);
  size_t pend_off[2] = {0, 0}, pend_n[2] = {0, 0};
  for (size_t off = 0, i = 0; off < total || pend_n[0] || pend_n[1]; i++) {
    gel_problem::Slot& sl = p->slot[i & 1];
    if (pend_n[i & 1]) {
      HIPCHK(hipStreamSynchronize(sl.stream.get()));
      par_copy(J + pend_off[i & 1], sl.h_jv.get(), pend_n[i & 1] * 8);
      pend_n[i & 1] = 0;
    }
    if (off < total) {
      const size_t n = std::min(piece, total - off);
      HIPCHK(hipMemcpyAsync(sl.h_jv.get(), p->jfd.J.get() + off, n * 8, hipMemcpyDeviceToHost, sl.stream.get()));
      pend_off[i & 1] = off; pend_n[i & 1] = n;
      off += n;
    }
  }
  return p->jfd.status;
}

int gel_jac_fd(gel_problem* p, int32_t group, const double* x, double* J) { return jfd_host(p, group, x, J, 0); }

int gel_jac_fd_blocks(gel_problem* p, int32_t group, const double* x, double* blocks) { return jfd_host(p, group, x, blocks, 1); }

int gel_jac_fd_block_dims(const gel_problem* p, int32_t group, int64_t* rows, int64_t* cols, int64_t* row0, int64_t* offset) {
  if (!p || group < 0 || group >= GEL_NUM_GROUPS) return fail(GEL_ERR_ARG, "bad argument");
  int64_t off = 0;
  for (int i = 0; i < p->dims.S; i++) {
    const int64_t r = (int64_t)jfd_w(group) * p->ph[i].n, c = 13 * (int64_t)p->ph[i].n + 13;
    if (rows) rows[i] = r;
    if (cols) cols[i] = c;
    if (row0) row0[i] = (int64_t)jfd_w(group) * p->ph[i].ua;
    if (offset) offset[i] = off;
    off += r * c;
  }
  if (offset) offset[p->dims.S] = off;
  return GEL_OK;
}

int gel_jac_fd_block_cols(const gel_problem* p, int32_t phase, int32_t* cols) {
  if (!p || !cols || phase < 0 || phase >= p->dims.S) return fail(GEL_ERR_ARG, "bad argument");
  std::vector<int32_t> c;
  phase_columns(p, phase, c);
  std::memcpy(cols, c.data(), sizeof(int32_t) * c.size());
  return GEL_OK;
}

int gel_jac_fd_device(gel_problem* p, int32_t group, const double* d_x, double* d_J, int32_t blocks, void* stream) {
  if (!p || !d_x || !d_J || group < 0 || group >= GEL_NUM_GROUPS) return fail(GEL_ERR_ARG, "bad argument");
  NEED_DEVICE(p, GEL_ERR_HIP, kNoGpu);
  HIPCHK(hipSetDevice(p->device));
  int rc = jfd_allocate(p);
  if (rc) return rc;
  hipStream_t s = stream_of(p, stream);
  p->jfd.last_x.clear();   // the residuals kept for gel_jac_fd's host callers are overwritten
  if ((rc = jfd_evaluate(p, d_x, s))) return rc;
  size_t total = 0;
  return jfd_quotients(p, group, blocks ? 1 : 0, d_J, s, &total);
}

// --------------------------- RHS / point hooks ---------------------------
static int need_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(GEL_ERR_HIP, "no HIP device: the engine has no CPU fallback");
  return GEL_OK;
}

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

static size_t aero_jac_len(const gel_problem* p, int kind) { return p->aero.rows[kind].size() * ((kind == 1) ? 8 : 12); }

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

// Vectors per slab of a call (what gel_prop_plan_info reports): as many as the workspace cap holds, a multiple of 64; or
// GEL_PROP_SLAB (measurement switch, read per call, rounded up to a multiple of 64; a value above the cap is ignored).  The
// results do not depend on it.
static int64_t prop_slab(const gel_prop_plan* pl) {
  const int64_t per_vec = 16 * pl->sampled_pts;
  int64_t vs = per_vec ? std::min<int64_t>(kPropMaxSlab, kPropWsBytes / per_vec / 64 * 64) : kPropMaxSlab;
  if (vs < 64) vs = 64;   // (a host-only handle's plan may hold more stage points than a device handle's: creation refuses those there)
  if (const char* e = getenv("GEL_PROP_SLAB")) {
    const long long w = (atoll(e) + 63) / 64 * 64;
    if (w >= 64 && w <= vs) vs = w;
  }
  return vs;
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

// ------------- wind ensemble of a Monte-Carlo batch -------------
// E member tables, each staged like a handle's own wind table, resident in device memory, and one assignment member [B] that the
// flight (gel_propagate_ensemble*) and the table (gel_output_table_batch_ensemble*) of a batch read alike.  It refers to the source
// handle for the device and the stream and is destroyed before it.
struct gel_wind_ensemble {
  gel_problem* src = nullptr;
  int32_t E = 0, Kw = 0;
  int64_t stride = 0;             // doubles per member: 5 Kw - 2
  std::vector<double> staged;     // [E][stride]: rows | slopes of every member (gel_wind_ensemble_member)
  int32_t assigned = -1;          // vectors of the current assignment, -1 before the first
  DeviceArray<double> d_tables;
  DeviceArray<int32_t> d_member;
};

// what a call hands its launches: nothing without an ensemble; v0 = the first vector of the slab
static gel::EnsDev ens_dev(const gel_wind_ensemble* ens, int64_t v0) {
  gel::EnsDev e{};
  if (!ens) return e;
  e.tables = ens->d_tables.get(); e.member = ens->d_member.get() + v0;
  e.E = ens->E; e.Kw = ens->Kw; e.stride = ens->stride;
  return e;
}
// an evaluation call's ensemble: of the same source handle, and assigned exactly the call's B vectors
static int ens_check(const char* what, const gel_wind_ensemble* ens, const gel_problem* src, int32_t B) {
  if (!ens) return GEL_OK;
  if (ens->src != src) return fail(GEL_ERR_ARG, std::string(what) + ": the wind ensemble belongs to another handle");
  if (ens->assigned != B)
    return fail(GEL_ERR_ARG, std::string(what) + ": the wind ensemble is assigned " +
                                 (ens->assigned < 0 ? std::string("no vectors yet") : std::to_string(ens->assigned) + " vectors") +
                                 ", the call has B = " + std::to_string(B) + " (gel_wind_ensemble_assign)");
  return GEL_OK;
}

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
  if (plan->d_ws.capacity() < need) {
    HIPCHK(drain(p));   // an earlier call in flight, on the handle's stream or on the caller's, still reads the old block
    HIPCHK(plan->d_ws.reserve(need));
  }
  const size_t nv = (size_t)p->dims.num_vars, ny = (size_t)11 * p->dims.M, nd = (size_t)p->dims.S * GEL_PROP_NDISP;
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
  // (the ensemble's members and assignment are resident: the arena holds what it held)
  return staged_call(p, 0, {staged_in(x, (size_t)B * p->dims.num_vars), staged_out(y, (size_t)B * 11 * p->dims.M), staged_out(err, (size_t)B * p->dims.S * 4),
                            staged_in(disp, (size_t)B * p->dims.S * GEL_PROP_NDISP)},
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
  if (const char* e = getenv("GEL_PROP_SLAB")) {
    const long long w = (atoll(e) + 63) / 64 * 64;
    if (w >= 64 && w <= vs) vs = w;
  }
  return vs;
}

// the row count of the wind seeds and of gwind (gel_prop_wind_rows): every table a lane of the call may read fits
static int32_t prop_wind_rows(const gel_prop_plan* plan, const gel_wind_ensemble* ens) {
  return std::max<int32_t>(plan->src->dev.Kw, ens ? ens->Kw : 0);
}

// wind_call: one of gel_propagate_tangent_wind*, which take a third seed (dwind; NULL in the parents' calls)
static int proptan_check(const char* who, const gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const void* x, const void* dx,
                         const void* ddisp, const void* dwind, bool wind_call, const gel_wind_ensemble* ens, const void* y, const void* dy) {
  const std::string w(who);
  if (!plan) return fail(GEL_ERR_ARG, w + ": null plan");
  if (B < 0) return fail(GEL_ERR_ARG, w + ": B < 0");
  if (P < 1) return fail(GEL_ERR_ARG, w + ": P < 1");
  if ((int64_t)B * P > 0x7fffffffLL) return fail(GEL_ERR_ARG, w + ": B P exceeds 2^31 - 1 lanes");
  if (shared != 0 && shared != 1) return fail(GEL_ERR_ARG, w + ": shared is neither 0 nor 1");
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
  if (!plan || !info || B < 0 || P < 1 || (int64_t)B * P > 0x7fffffffLL || (shared != 0 && shared != 1))
    return fail(GEL_ERR_ARG, "gel_prop_tangent_info: bad argument");
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
  if (plan->d_ws.capacity() < need) {
    HIPCHK(drain(p));   // an earlier call in flight still reads the old block
    HIPCHK(plan->d_ws.reserve(need));
  }
  double* const ws = plan->d_ws.get();
  double* const dws = ws + (size_t)ldv * set;   // the second region: the seeds' samples
  // prop_sample_kernel alone: launch_prop_slab on a copy of the plan's tables that has no segment to integrate
  gel::PropDev sample_only = plan->dev;
  sample_only.chain = 0;
  sample_only.restart = 0;
  sample_only.nseg = 0;
  const size_t nv = (size_t)p->dims.num_vars, ny = (size_t)11 * p->dims.M, nd = (size_t)p->dims.S * GEL_PROP_NDISP;
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
  const size_t nv = (size_t)p->dims.num_vars, ny = (size_t)11 * p->dims.M, nd = (size_t)p->dims.S * GEL_PROP_NDISP;
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
  if (const char* e = getenv("GEL_PROP_SLAB")) {
    const long long w = (atoll(e) + 63) / 64 * 64;
    if (w >= 64 && w <= vs) vs = w;
  }
  return vs;
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
  if (plan->d_ws.capacity() < need) {
    HIPCHK(drain(p));   // an earlier call in flight still reads the old block
    HIPCHK(plan->d_ws.reserve(need));
  }
  double* const ws = plan->d_ws.get();
  double* const gws = ws + (size_t)ldv * set;    // the second region: the stage points' control multipliers
  double* const gS = gws + (size_t)gld * set;    // the third: the multiplier of S per (phase, lane)
  double* const ck = gS + (size_t)gld * (size_t)plan->dev.S;   // the fourth: the inner checkpoints of the interval in hand
  double* const gww = ck + (size_t)gld * nck + 1;              // the fifth: the lanes' wind columns [Kg][2][gld] (only where gwind is wanted)
  const size_t nv = (size_t)p->dims.num_vars, ny = (size_t)11 * p->dims.M, nd = (size_t)p->dims.S * GEL_PROP_NDISP;
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
  const size_t nv = (size_t)p->dims.num_vars, ny = (size_t)11 * p->dims.M, nd = (size_t)p->dims.S * GEL_PROP_NDISP;
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
  if (transpose && p->jp.d_tpart.capacity() < (size_t)B * p->dims.S * 2) {
    if (p->jp.d_tpart.get()) HIPCHK(drain(p));   // an earlier product in flight still sums through the old workspace
    HIPCHK(p->jp.d_tpart.reserve((size_t)B * p->dims.S * 2));
  }
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
    if (p->d_outws.capacity() < need) {
      HIPCHK(drain(p));   // an earlier call in flight still reads the old block
      HIPCHK(p->d_outws.reserve(need));
    }
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
  if (p->d_quantws.capacity() < L.bytes) {
    HIPCHK(drain(p));   // an earlier call in flight still uses the old block
    HIPCHK(p->d_quantws.reserve(L.bytes));
  }
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
  if (p->d_comws.capacity() < L.bytes) {
    HIPCHK(drain(p));   // an earlier call in flight still uses the old block
    HIPCHK(p->d_comws.reserve(L.bytes));
  }
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
  static const int nin[16] = {1, 3, 3, 6, 7, 1, 1, 2, 2, 8, 8, 8, 7, 4, 1, 5}, nout[16] = {5, 3, 3, 3, 3, 3, 1, 4, 6, 8, 16, 4, 3, 7, 2, 18};
  if (kind < 0 || kind > 15 || n < 0 || !in || !out) return fail(GEL_ERR_ARG, "bad argument");
  if (n == 0) return GEL_OK;
  const bool tabulated = kind == 5 || kind == 6 || kind == 9 || kind == 10 || kind == 15;
  int rc = tabulated ? check_launch_lds("gel_point_eval", gel::point_lds_bytes(aux_rows), 5 * (size_t)std::max(aux_rows, 0), 5 * (size_t)std::max(aux_rows, 0), false) : GEL_OK;
  if (rc) return rc;
  rc = need_device();
  if (rc) return rc;
  double atm[gel::kAtmTableDoubles];
  size_t naux = 0;
  const double* hax = aux;
  std::vector<double> ext;  // kinds 5 / 6 / 9 / 10: the table rows followed by their per-interval slopes; kind 15: the atmosphere table before them
  if (kind == 0) { gel::fill_atmosphere_table(atm); hax = atm; naux = gel::kAtmTableDoubles; aux_rows = 0; }
  else if (kind == 2) { if (!aux) return fail(GEL_ERR_ARG, "kind 2 needs aux[0] = barC20"); naux = 1; aux_rows = 0; }
  else if (tabulated) {
    const int w = (kind == 5 || kind == 10 || kind == 15) ? 3 : 2;
    if (!aux || aux_rows < 2) return fail(GEL_ERR_ARG, "kinds 5, 6, 9, 10 and 15 need a table of at least two rows");
    if (kind == 15) { gel::fill_atmosphere_table(atm); ext.assign(atm, atm + gel::kAtmTableDoubles); }   // atmosphere | wind rows | slopes
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
