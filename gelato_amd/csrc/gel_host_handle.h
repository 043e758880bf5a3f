// gel_host_handle.h -- the handle (struct gel_problem) and what more than one of the host files that make HIP calls needs, and nothing
// else: the owners of device and pinned memory, the handle's streams, the launch-limit checks, the launches an exact-Jacobian flag
// reroutes, the staged host-buffer call and the wind ensemble.  gel_host_lgr.hip makes no HIP call and has no handle: it includes
// gel_host_internal.h alone.  As there, everything lives in namespace gelhost under hidden visibility (the C surface's opaque types
// gel_problem and gel_wind_ensemble keep their global names) and nothing sits in an anonymous namespace: the handle is one and the
// same type in every translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "gel_device.h"
#include "gel_launch.h"
#include "gel_mesh.h"
#include "gel_jprod.h"
#include "gel_conprod.h"
#include "gel_ensemble.h"
#include "gel_host_internal.h"

#pragma GCC visibility push(hidden)

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(GEL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

// A workspace that only grows: what is in flight, on the handle's stream or on the caller's, still uses the old block, so the drain
// comes before the reserve.  A macro, so that the message of a failed reserve names the member, as every HIPCHK message does.
#define GROW_AFTER_DRAIN(p, arr, need)     \
  do {                                     \
    if (arr.capacity() < (need)) {         \
      HIPCHK(drain(p));                    \
      HIPCHK(arr.reserve(need));           \
    }                                      \
  } while (0)

namespace gelhost {

// The only owners of device and pinned memory in the host files: an array frees its block in its destructor (and when it is
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

struct HostPhase {
  int n, ua, xa;
  int air, air_fd, t_fd, q_fd, engine_on, hold;
  int K, s_vv, s_vq, s_vt, s_qq;
  int64_t voff;
  double thrust, massflow, area, nozzle;
  std::vector<double> D, tau;
};

}  // namespace gelhost

using gelhost::DeviceArray;
using gelhost::HostPhase;
using gelhost::PinnedArray;
using gelhost::Stream;

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

namespace gelhost {

// kind: 0 = constant value; 1 = x-dependent, value = compact[slot]; 2 = x-dependent, value = -compact[slot]
// (slot = compact index within the eval; several entries may name the same slot)
using Visitor = std::function<void(int block, int64_t k, int32_t row, int32_t col, int kind, double cval, int64_t slot)>;
// walks all 13 blocks in the reference's emission order; k is the index inside the block (gel_host.hip)
void walk_pattern(const gel_problem& P, const Visitor& vis);
// appends the global column of every local column of phase i as a one-phase problem (gel_host_fd.hip)
void phase_columns(const gel_problem* p, int i, std::vector<int32_t>& colmap);
// the operator tables of the Jacobian products, at gel_problem_create: a message on a pattern they do not cover, else null (gel_host_jprod.hip)
const char* build_jprod_tables(gel_problem& P);

// Caller-owned streams (gel_host.hip).  stream_of: the stream a device-form entry point launches on, the caller's
// (remembered for drain) or, for NULL, the handle's own.  drain: before device memory that launches read or write is released or
// replaced, wait for the handle's own stream AND for the last caller-owned one.  clear_flag: clear the device's non-finite flag
// and WAIT for the clear.
hipStream_t stream_of(gel_problem* p, void* stream);
hipError_t drain(gel_problem* p);
hipError_t clear_flag(gel_problem* p, hipStream_t s);

// A host-only handle is refused with the code and the text of the entry point's family.
#define NEED_DEVICE(p, code, text)                                  \
  do {                                                              \
    if ((p)->device == GEL_DEVICE_NONE) return fail(code, text);    \
  } while (0)
constexpr const char* kNoGpu = "host-only handle: nothing can be evaluated without a GPU (no CPU fallback)";
// GEL_OK, or GEL_ERR_HIP where the machine has no HIP device (the entry points that take no handle)
int need_device();

// The launch-limit checks (gel_host.hip): a workgroup of a launch that stages the tables may take gel::kLaunchMaxLds bytes; the host
// decides with the launchers' own sizes, before anything is enqueued.
// lds_room: the table doubles that fit beside `rest` doubles of other LDS (padded: the rest starts at an even double)
size_t lds_room(size_t rest, bool padded);
// GEL_OK, or GEL_ERR_ARG with the table doubles asked for and those that fit; `staged` = the doubles the tables take in the launch
int check_launch_lds(const char* what, size_t lds_bytes, size_t asked, size_t staged, bool padded);
int check_table_launches(int Kw, int Kc);

// The launches that a handle's exact-Jacobian flags reroute.  Inline: the one-vector path (gel_host.hip) and the batch entry points
// (gel_host_constraints.hip) both call them, and the former keeps every call it makes in its own translation unit.
// The defect groups of B vectors: one launch of the fused kernel; on a handle created with GEL_FLAG_EXACT_DEFECT_JAC, a call with
// derivatives is the residual-only launch of the fused kernel (when residuals are asked for) followed by the exact-Jacobian kernel.
inline hipError_t launch_defects(const gel_problem* p, const gel::ProblemDev& dv, int B, const double* x, double* res, double* jvar,
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
inline hipError_t launch_aero_kinds(const gel_problem* p, const gel::ProblemDev& dv, int nnodes, const gel::AeroNodeDev* nodes, int B,
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
inline hipError_t launch_rows_kinds(const gel_problem* p, const gel::ProblemDev& dv, int B, const double* x, double* con, double* jfn,
                                    hipStream_t s) {
  const int nlin = (int)p->lin_rows.size(), nfn = (int)p->fn_rows.size();
  if (!p->exact_rows || !jfn) return gel::launch_rows(dv, nlin, p->d_lin_rows.get(), nfn, p->d_fn_rows.get(), B, x, con, jfn, s);
  const hipError_t e = gel::launch_rows(dv, nlin, p->d_lin_rows.get(), nfn, p->d_fn_rows.get(), B, x, con, nullptr, s);
  if (e != hipSuccess) return e;
  return gel::launch_rows_exact(dv, nfn, p->d_fn_rows.get(), B, x, jfn, s);
}
inline size_t aero_jac_len(const gel_problem* p, int kind) { return p->aero.rows[kind].size() * ((kind == 1) ? 8 : 12); }

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

// the two pinned staging slots of the pipelined host batch, which also carry gel_jac_fd's result back; memcpy on a few threads (gel_host.hip)
int ensure_slots(gel_problem* p);
void par_copy(void* dst, const void* src, size_t bytes);

// what a call hands its launches: nothing without an ensemble; v0 = the first vector of the slab
inline gel::EnsDev ens_dev(const gel_wind_ensemble* ens, int64_t v0) {
  gel::EnsDev e{};
  if (!ens) return e;
  e.tables = ens->d_tables.get(); e.member = ens->d_member.get() + v0;
  e.E = ens->E; e.Kw = ens->Kw; e.stride = ens->stride;
  return e;
}
// an evaluation call's ensemble: of the same source handle, and assigned exactly the call's B vectors
int ens_check(const char* what, const gel_wind_ensemble* ens, const gel_problem* src, int32_t B);   // (gel_host_flight.hip)

}  // namespace gelhost

#pragma GCC visibility pop
