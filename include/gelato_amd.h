/*
 * gelato_amd.h -- C-ABI of the MI355X-native LGR defect-residual / FD-Jacobian engine.
 *
 * This is the drop-in boundary for GELATO's hot path.  In the reference that
 * path is reached from pyoptsparse's objfunc/sens callbacks
 * (Trajectory_Optimization.py:194-312) through eight Python functions of
 * lib/con_dynamics.py and, below them, the pybind11 module `dynamics_c`
 * (src/pybind_dynamics.cpp:108-114) plus NumPy's D.dot(X).  Each entry point
 * below names the reference interface it replaces.  Plain pointers and sizes
 * only; the caller owns every buffer it passes; the engine owns device memory.
 * One handle = one HIP device + one HIP stream; a handle is not thread-safe.
 *
 * Streams.  The sixteen entry points with a `void* stream` parameter (the *_device forms and gel_sync) enqueue everything they
 * do -- every launch, memset and use of a workspace of the handle -- on that stream, a hipStream_t of the caller (blocking or
 * not) or NULL for the handle's own; every other call runs on the handle's own stream and returns synchronised.  The calls of
 * ONE handle must not overlap on different streams (two handles on two streams may): order them on one stream, or gel_sync
 * between them.  The non-finite status is per handle, not per stream: it is read and cleared by gel_sync on the stream the
 * calls were given, and a host-form call made while device-form work is still pending may report and clear that work's status.
 * The handle remembers the last caller stream it was given until gel_sync on it returns; whatever releases device memory that
 * launches read -- gel_aero_configure, gel_rows_configure, gel_shard_plan, a workspace or staging buffer that has to grow --
 * first waits for the handle's own stream AND for that stream, so a reconfiguration behind pending work is safe (and blocks the
 * host until that work is done).  A caller's stream must stay valid until gel_sync on it has returned.
 *
 * Packed decision vector x (all normalised by `units`, doubles) -- exactly the
 * concatenation of the reference's xdict arrays
 * (Trajectory_Optimization.py:318-352):
 *     [ mass M | position 3M | velocity 3M | quaternion 4M | u 2N | t S+1 ]
 * with S phases, N = sum(num_nodes), M = N + S.
 *
 * Residual vector (11N doubles): [ eqcon_dyn_mass N | eqcon_dyn_pos 3N |
 * eqcon_dyn_vel 3N | eqcon_dyn_quat 4N ], each exactly as
 * lib/con_dynamics.py:63,152,289,533 returns it.
 *
 * Jacobian values: 13 COO blocks in the order
 *   group 0 eqcon_dyn_mass : mass, t
 *   group 1 eqcon_dyn_pos  : position, velocity, t
 *   group 2 eqcon_dyn_vel  : mass, position, velocity, quaternion, t
 *   group 3 eqcon_dyn_quat : quaternion, u, t
 * each in the reference's exact emission order (lib/con_dynamics.py:66-113,
 * 155-213,292-496,536-632).  "full" = all 13 blocks
 * concatenated; "compact" = the DISTINCT x-dependent values (everything that is
 * not a constant D / 0 / +-1 / massflow entry; a tf column that is the exact
 * negative of its t0 column, and the node-uniform pos/velocity diagonal value,
 * are held once), in the engine's coalesced device order, mapped into "full" by
 * the gather map gel_full_source().
 *
 * Status codes: 0 = ok; GEL_NONFINITE (1) = the evaluation completed but some
 * output is NaN/Inf (the Python shim maps it to pyoptsparse's fail=True; the
 * reference itself hard-codes fail=False, Trajectory_Optimization.py:240,311);
 * negative = error (bad argument, HIP failure).  gel_last_error() gives text.
 */
#ifndef GELATO_AMD_H_
#define GELATO_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEL_OK 0
#define GEL_NONFINITE 1
#define GEL_ERR_ARG (-1)
#define GEL_ERR_HIP (-2)
#define GEL_ERR_ALLOC (-3)

#define GEL_DEVICE_NONE (-1) /* gel_problem_desc.device: host-only handle (pattern / dims / LGR), cannot evaluate */

/* gel_problem_desc.flags */
#define GEL_FLAG_DX_MFMA 1 /* force the D.X product onto v_mfma_f64_16x16x4_f64 */
#define GEL_FLAG_DX_VALU 2 /* force wavefront dot-products (VALU FMAs) */
#define GEL_FLAG_NO_PACK 4 /* matrix-pipe form of a problem whose phases all have <= 32 nodes: one decision vector per
                              wavefront (32 idle lanes) instead of two -- for A/B measurements and parity tests */
#define GEL_FLAG_ITEM_MAJOR 16 /* cooperative launches in work-item major order also when every phase has at most 32 nodes (the default there is
                              vector-group major, XCD-aware: see gel_eval_kernel.h) -- for A/B measurements */
#define GEL_FLAG_FD_RECOMPUTE 8 /* every finite-difference sweep re-runs the reference's chain on the perturbed input
                              (lib/con_dynamics.py:381-400,452-480), as rounds 1-2 did.  Default (flag clear): the three position
                              sweeps form the CHANGE of altitude / atmosphere / wind from algebraic difference identities of the
                              reference's formulas (accurate to ~1e-12 of the change, where a recomputation carries the
                              reference's own 1e-8 .. 1e-4 finite-difference noise), and the t0 / tf columns of aerodynamic
                              phases are written in closed form +-f_c unit_t/2 (the RHS does not depend on t; the reference's two
                              sweeps only add rounding noise, <= 2e-6 measured).  Both forms meet the stated tolerance against
                              the reference's values; with the flag set the compact layout keeps separate t0 / tf slots. */
#define GEL_FLAG_EXACT_DEFECT_JAC 32 /* opt-in: every x-dependent entry of the reference's pattern for the four defect groups'
                              Jacobians (equality_jac_dynamics_{mass,position,velocity,quaternion}) is the analytic derivative of the
                              residual the handle computes, formed in fp64 forward mode (value plus tangent along each variable) --
                              exact to rounding, where the default is the reference's forward difference.  dx is ignored for these
                              groups.  Exact ON THE REFERENCE'S PATTERN: where the pattern has no slot for a dependence, none is
                              added -- a phase with reference_area < 0 depends on velocity through the aerodynamic force, but the
                              reference's pattern holds only D there (no velocity sweep, lib/con_dynamics.py:403), and so does this.
                              The aero path constraints' gradients (gel_eval_aero*, the callback's aero part) and the node-function
                              rows (gel_rows_*, the callback's row table) STAY forward differences with dx; GEL_FLAG_EXACT_AERO_JAC
                              (64) makes the aero part exact as well, GEL_FLAG_EXACT_ROWS_JAC (128) the node-function rows.
                              Residuals are bit-identical to a handle without the flag (the fused kernel's residual-only form runs
                              first; the exact kernel then writes the compact Jacobian: two launches per evaluation; gel_eval_callback
                              runs them, then the row table and the aero kinds, in launches of their own).  Pattern,
                              constants, compact layout and gather map are those of the default layout.  Evaluates through
                              gel_eval_residual / _jacobian, gel_eval, gel_eval_batch, gel_eval_batch_device, gel_eval_full_device and
                              gel_eval_callback; gel_eval_batch_aero_device (unless GEL_FLAG_EXACT_AERO_JAC is set as well) and
                              gel_eval_shard_* return GEL_ERR_ARG, and so does
                              gel_problem_create for GEL_FLAG_FD_RECOMPUTE | GEL_FLAG_EXACT_DEFECT_JAC (or |dx * unit_position| > 1),
                              also on a host-only handle.  Conventions where the value is not differentiable -- the derivative of
                              the branch the value took: the table interval used (0 where interp clamps, x <= xp[0] included), the
                              atmosphere layer and the 86 km geopotential switch, the gravity r < b clamp; air-relative speed 0:
                              d|v_air| = 0 (the force's derivative is 0 there); polar axis p = 0: the partials of p and of the
                              longitude are 0.  A non-finite entry it writes makes the call return GEL_NONFINITE (gel_sync for the
                              device forms). */
#define GEL_FLAG_EXACT_AERO_JAC 64 /* opt-in, independent of GEL_FLAG_EXACT_DEFECT_JAC (either alone or both): every gradient entry the
                              aero path constraints write (angle of attack, dynamic pressure, q-alpha: inequality_jac_max_*) is the
                              analytic derivative of con = 1 - f / limit with respect to the normalised position, velocity and
                              quaternion (quaternion for alpha and q-alpha only), formed in fp64 forward mode -- exact to rounding,
                              where the default is the reference's forward difference with dx.  The t0 / tf columns are exact zeros
                              (the air-relative velocity does not depend on the Earth angle).  Dims, pattern, record layout and
                              record map (gel_aero_dims / _pattern / _record_layout / _record_map) are those of the default.  The
                              constraint values are bit-identical to a handle without the flag: the values-only aero launch runs
                              first, then the exact kernel (gel_kernels_exact_aero.hip) writes the gradients.  Honoured by
                              gel_eval_aero, gel_eval_aero_all, gel_eval_aero_all_device, gel_eval_callback (aero part in launches of
                              its own) and gel_eval_batch_aero_device (defect groups as gel_eval_batch_device forms them, then both
                              parts of the record; not the fused form).  gel_problem_create returns GEL_ERR_ARG for
                              GEL_FLAG_FD_RECOMPUTE | GEL_FLAG_EXACT_AERO_JAC (or |dx * unit_position| > 1: the t columns are laid
                              out differently there), also on a host-only handle.  Conventions: alpha's entries are 0 where its value
                              is clamped to 0 (cos(alpha) > 1 or |v_air|^2 < 1e-12) and where the air velocity and the body axis are
                              exactly parallel; the table-interval, atmosphere-layer, polar-axis and zero-air-speed conventions are
                              those of GEL_FLAG_EXACT_DEFECT_JAC.  A non-finite entry it writes makes the call return GEL_NONFINITE
                              (gel_sync for the device forms).  The node-function rows stay forward differences unless
                              GEL_FLAG_EXACT_ROWS_JAC (128) is set as well. */
#define GEL_FLAG_EXACT_ROWS_JAC 128 /* opt-in, combines with every other flag (GEL_FLAG_FD_RECOMPUTE included: the jfn layout does not
                              depend on any flag): every jfn entry of a node-function row (gel_rows_configure: the terminal orbit
                              rows, the device-form user constraints, the waypoint / impact-point / antenna / downrange rows) is
                              s (df / dx_c) / p[0], s = -1 with mode & 8, for every value mode and for mode & 4 alike (their forward
                              differences all approximate this quantity): the analytic derivative of the row's function with
                              respect to the normalised column c (0..2 position, seed unit_position; 3..5 velocity, unit_velocity;
                              6 the knot time, unit_t, where tcol >= 0), formed in fp64 forward mode -- exact to rounding, where
                              the default is the forward difference with dx.  Columns the function does not read are exact zeros:
                              column 6 of fn 0..8 and of rows with tcol < 0, the velocity columns of fn 9..11, 14 and 15.  The row
                              values are bit-identical to a handle without the flag: rows_kernel runs without its jfn output, then
                              the exact kernel (gel_kernels_exact_rows.hip) writes jfn.  Honoured by gel_rows_eval,
                              gel_rows_eval_device and gel_eval_callback (the row table in launches of its own when rows_jfn is
                              asked for).  Conventions where the value is not differentiable -- the derivative of the branch the
                              value took: an impact point without a solution (the (0, 0) fill) has all seven entries 0; the
                              inclination where c_z / |c| = +-1 exactly: 0; a norm at exactly 0 (|c|, e, |r|, |v|): its tangent is
                              0; polar axis p = 0: the partials of p and of the longitude are 0; Vincenty with lon2 - lon1 == 0
                              exactly: 0, otherwise the tangent carried through its loop, whose exit the value decides.  A
                              non-finite entry it writes makes the call return GEL_NONFINITE (gel_sync for the device form). */

#define GEL_NUM_GROUPS 4
#define GEL_NUM_BLOCKS 13

typedef struct gel_problem gel_problem; /* opaque */

/* Static problem = the hot path's view of pdict + unitdict
 * (Trajectory_Optimization.py:116-167): per-phase event parameters
 * (lib/con_dynamics.py:249-252,46-61,521), units, dx, wind and CA tables. */
typedef struct {
  int32_t num_sections;          /* S  (pdict["num_sections"]) */
  const int32_t* num_nodes;      /* [S] LGR nodes per phase (events["num_nodes"]) */
  const double* thrust;          /* [S] vacuum thrust, N          (params[i]["thrust"]) */
  const double* massflow;        /* [S] kg/s                      (params[i]["massflow"]) */
  const double* reference_area;  /* [S] m^2; == 0 selects the NoAir RHS (con_dynamics.py:257) */
  const double* nozzle_area;     /* [S] m^2                       (params[i]["nozzle_area"]) */
  const int32_t* engine_on;      /* [S] params[i]["engineOn"] */
  const int32_t* attitude_hold;  /* [S] 1 iff params[i]["attitude"] in ("hold","vertical") */
  double unit_mass, unit_position, unit_velocity, unit_u, unit_t; /* unitdict */
  double dx;                     /* pdict["dx"], 1e-8 in the reference */
  double barC20;                 /* normalised C20 of the J2 gravity; 0 -> -0.484165371736e-3 (src/gravity.cpp:18) */
  int32_t wind_rows;             /* K */
  const double* wind_table;      /* [K][3] altitude, wind_n, wind_e (pdict["wind_table"]) */
  int32_t ca_rows;
  const double* ca_table;        /* [K][2] Mach, CA (pdict["ca_table"]) */
  const double* D;               /* optional: per-phase D (n x (n+1), row-major) concatenated, i.e.
                                    pdict["ps_params"].D(i); NULL -> generated by gel_lgr_diffmat */
  const double* tau;             /* optional: per-phase tau concatenated; NULL -> gel_lgr_nodes */
  int32_t device;                /* HIP device ordinal */
  int32_t flags;                 /* 0 or GEL_FLAG_* */
} gel_problem_desc;

typedef struct {
  int32_t S, N, M;
  int32_t num_vars;              /* 11M + 2N + S + 1 */
  int32_t num_rows[GEL_NUM_GROUPS]; /* N, 3N, 3N, 4N */
  int64_t block_nnz[GEL_NUM_BLOCKS];
  int64_t block_shape[GEL_NUM_BLOCKS][2];
  int64_t total_nnz;             /* "full" length */
  int64_t num_var_entries;       /* "compact" length V */
  int64_t algorithmic_bytes;     /* SURVEY.md 8(d) A_min per eval: 8*(num_vars + 11N + V_ref), V_ref = every x-dependent
                                    value the reference computes (9n + 39n|30n + 32n per phase) */
  int64_t stored_bytes;          /* what one eval writes: 8*(11N + V) */
} gel_dims;

/* ---- LGR transcription on the host (replaces lib/PSfunctions.py:149-168,182-208,
 *      i.e. nodes_LGR(n) and differentiation_matrix_LGR(n), reverse=True) ---- */
int gel_lgr_nodes(int32_t n, double* tau /* [n] */);
int gel_lgr_diffmat(int32_t n, double* D /* [n][n+1] */);

/* ---- problem life cycle (replaces building pdict["ps_params"] + the static
 *      part of every con_dynamics call) ---- */
int gel_problem_create(const gel_problem_desc* desc, gel_problem** out);
int gel_problem_destroy(gel_problem* p);
int gel_problem_dims(const gel_problem* p, gel_dims* out);
int gel_problem_D(const gel_problem* p, int32_t phase, double* D);     /* PSparams.D(i),   SectionParameters.py:46-49 */
int gel_problem_tau(const gel_problem* p, int32_t phase, double* tau); /* PSparams.tau(i), SectionParameters.py:41-44 */

/* ---- fixed sparsity pattern (what the first sens() call hands to
 *      addConGroup(jac=...), Trajectory_Optimization.py:354-355,400-407) ---- */
int gel_pattern(const gel_problem* p, int32_t block, int32_t* rows, int32_t* cols); /* block 0..12 */
int gel_pattern_all(const gel_problem* p, int32_t* rows_full, int32_t* cols_full);  /* all 13 blocks concatenated ("full"), one pass */
int gel_const_values(const gel_problem* p, double* vals_full); /* constants filled, x-dependent entries 0 */
int gel_var_index(const gel_problem* p, int64_t* idx /* [V] compact slot -> index into full (its first plain use) */);
/* the gather map full <- compact: src[i] = -1: constant (gel_const_values); s >= 0: compact[s]; s <= -2: -compact[-2 - s] */
int gel_full_source(const gel_problem* p, int32_t* src /* [total_nnz] */);

/* ---- evaluation, host buffers (B = 1; the pyoptsparse callback path) ----
 * gel_eval_residual : equality_dynamics_{mass,position,velocity,quaternion}
 *                     (lib/con_dynamics.py:34,116,216,499) in one launch.
 * gel_eval_jacobian : equality_jac_dynamics_{...} (lib/con_dynamics.py:66,155,292,536)
 *                     in one launch.  vals_full must be a buffer of total_nnz
 *                     doubles; if fill_constants != 0 the constant entries are
 *                     (re)written too, otherwise only the x-dependent entries are
 *                     touched (the buffer is assumed to still hold the constants).
 * gel_eval          : both at once (one objfunc + one sens share of the hot path). */
int gel_eval_residual(gel_problem* p, const double* x, double* res);
int gel_eval_jacobian(gel_problem* p, const double* x, double* vals_full, int32_t fill_constants);
int gel_eval(gel_problem* p, const double* x, double* res, double* vals_full, int32_t fill_constants);

/* ---- evaluation, batched over B decision vectors ----
 * host buffers: x [B][num_vars], res [B][11N], jvar [B][V] (compact). */
int gel_eval_batch(gel_problem* p, int32_t B, const double* x, double* res, double* jvar);
/* device buffers (inputs already resident in HBM; asynchronous on `stream`,
 * which is a hipStream_t or NULL for the handle's own stream).  res may be NULL
 * (Jacobian only is not offered: the centre RHS is shared); jvar may be NULL
 * (residual only).  Returns after enqueueing; call gel_sync() for the status. */
int gel_eval_batch_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, void* stream);
/* materialise every COO value like the reference does: d_jfull [B][total_nnz],
 * from d_jvar [B][V] (compact -> full expansion kernel). */
int gel_expand_full_device(gel_problem* p, int32_t B, const double* d_jvar, double* d_jfull, void* stream);
/* The handle's own pinned host buffers for the one-vector calls (gel_eval_residual, gel_eval, gel_eval_jacobian,
 * gel_eval_callback): *res [11N] and *vals_full [total_nnz, the constants already in place].  A caller that passes THESE pointers
 * as its res / vals_full gets its results without a host copy: the kernel writes the residual rows and every block of the value
 * vector whose entries are all x-dependent straight to their places (COO-direct output, gelato_amd/csrc/gel_eval_kernel.h), and
 * the host only scatters the entries that sit alone between constants.  The buffers belong to the handle and are rewritten by the
 * next such call (the reference returns fresh arrays, lib/con_dynamics.py:108-113; pyoptsparse copies what it is given at once).
 * *x0, *x1 [num_vars]: two pinned decision-vector buffers; a one-vector call whose x is one of them reads it in place (two, so that a
 * caller can keep the previous vector for comparison while it fills the next).  Any of the four out-pointers may be NULL. */
/* One-vector calls (gel_eval, gel_eval_jacobian, gel_eval_callback) return when the kernel itself has told the host that its results
 * are in the pinned buffers (its last workgroup stores a sequence number there after every workgroup's system-scope release), 4-5 us
 * before the runtime's end-of-kernel signal; the handle's stream may still hold the kernel's tail, and whatever is launched on it
 * next is ordered behind.  Environment GEL_DONE_FLAG=0: wait for the runtime's signal instead. */
int gel_pinned_buffers(gel_problem* p, double** res, double** vals_full, double** x0, double** x1);
/* The same result without rewriting the constants (the reference rebuilds every COO value per call,
 * lib/con_dynamics.py:108-111,491-494,627-630): gel_fill_full_device lays the constant template into d_jfull [B][total_nnz]
 * ONCE, gel_update_full_device then writes only the x-dependent entries (4 % of the values at 6 x 64) from d_jvar [B][V] after
 * every evaluation.  Bit-identical to gel_expand_full_device as long as nothing else writes the buffer. */
int gel_fill_full_device(gel_problem* p, int32_t B, double* d_jfull, void* stream);
int gel_update_full_device(gel_problem* p, int32_t B, const double* d_jvar, double* d_jfull, void* stream);
/* One evaluation with EVERY COO value valid in HBM afterwards: the fused launch (d_res may be NULL) followed by the update of
 * d_jfull [B][total_nnz] (laid down once by gel_fill_full_device) from the compact values it has just written to d_jvar [B][V].
 * A launch whose output fits the Infinity Cache writes the compact values with ordinary instead of non-temporal stores, so that
 * the update finds them there (6 x 64, B = 1024: 0.26 -> 0.165 ms, 6.2 M evals/s).  Same bits as gel_eval_batch_device +
 * gel_update_full_device. */
int gel_eval_full_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, double* d_jfull, void* stream);
/* multi-GPU sharding of ONE batch (the defect path is block-diagonal per phase, lib/con_dynamics.py:46,132,237,320,512,554,
 * and its forward-difference columns are independent).  A work item = one 64-node chunk of one phase;
 * unit = 4 * work_item + part, part 0 = everything of the work item except its three position
 * sweeps, parts 1..3 = one position sweep each (empty for phases without aerodynamics), i.e. the forward-
 * difference COLUMNS of lib/con_dynamics.py:381-400 dealt to different GPUs (BASELINE.json configs[3]).  A unit
 * writes only its own entries of d_res / d_jvar; disjoint unit ranges compose to the full evaluation.  d_jvar is
 * required; d_res may be NULL. */
int gel_eval_shard_units_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar,
                                int32_t unit_begin, int32_t unit_count, void* stream);
/* which unit writes which output entry: res_owner [11N], jvar_owner [V] (unit ids as above).  With it ranks owning disjoint
 * unit ranges exchange exactly their own entries (one all-gather, gelato_amd/parallel.py) instead of reducing full buffers. */
int gel_unit_owner(const gel_problem* p, int32_t* res_owner, int32_t* jvar_owner);
/* Packed exchange of a unit-sharded evaluation: zero pack / unpack launches around the one collective.  gel_shard_plan fixes the
 * layout for `nranks` ranks holding the contiguous unit ranges [unit_begin[r], unit_begin[r+1]) (unit_begin[0] = 0,
 * unit_begin[nranks] = 4 * work items): ONE buffer out [nranks][B][width]; rank r's entries of vector b are the contiguous block
 * out[r][b][0 .. its share), every unit's entries one contiguous run inside it.  res_pos [11N] / jvar_pos [V] (either may be NULL)
 * = rank * width + offset of every entry of the ordinary res / compact-value layouts: entry i of vector b sits at
 * out[(pos / width) * B * width + b * width + pos % width].  gel_eval_shard_packed_device makes rank `rank`'s kernel write its
 * entries STRAIGHT into its slice out[rank] (all B vectors), so an in-place all-gather over the slices (send = out[rank],
 * receive = out) completes the buffer on every rank; a consumer reads it through the map, or asks
 * gel_shard_unpack_device for the ordinary layouts (one gather launch; d_res or d_jvar may be NULL).  A host-only handle can plan
 * (the CPU tests do); the plan is per handle and replaced by the next call -- which is why the two device calls take the
 * (nranks, width) the caller's buffer was sized for and return GEL_ERR_ARG when the handle holds another plan by now.
 * (lib/con_dynamics.py:46,132,237,320,512,554: per-phase independence; :381-400: independent forward-difference columns.) */
int gel_shard_plan(gel_problem* p, int32_t nranks, const int32_t* unit_begin /* [nranks + 1] */, int64_t* width,
                   int64_t* res_pos /* [11N] or NULL */, int64_t* jvar_pos /* [V] or NULL */);
int gel_eval_shard_packed_device(gel_problem* p, int32_t B, const double* d_x, double* d_out /* [nranks][B][width] */, int32_t rank,
                                 int32_t nranks, int64_t width, void* stream);
int gel_shard_unpack_device(gel_problem* p, int32_t B, const double* d_out, double* d_res, double* d_jvar, int32_t nranks,
                            int64_t width, void* stream);
int gel_num_chunks(const gel_problem* p, int32_t* nchunks);
int gel_chunk_phase(const gel_problem* p, int32_t* phase /* [nchunks] */);
/* which form of the fused kernel a launch of B vectors takes: info = {jacobian, D.X on the matrix pipe, split
 * latency form, wavefronts launched, two decision vectors per wavefront} -- so that a measurement can name the kernel
 * it timed. */
int gel_launch_info(const gel_problem* p, int32_t B, int32_t want_res, int32_t want_jac, int32_t* info /* [5] */);
int gel_sync(gel_problem* p, void* stream); /* waits; returns GEL_NONFINITE if any eval since the last sync produced NaN/Inf */

/* ---- generic column-batched dense forward difference (replaces lib/jac_fd.py:29-62
 *      applied to the four defect residuals; used as the cross-check of the
 *      structured Jacobians).  J [num_rows[group]][num_vars], row-major. ---- */
int gel_jac_fd(gel_problem* p, int32_t group, const double* x, double* J);
/* The same quotients without the zeros.  Each phase's rows see only the phase's own 13 n + 13 columns (every other column of
 * the reference's dense result, lib/jac_fd.py:54-60, is an exact zero): block i = [rows[i] = w n_i][cols[i] = 13 n_i + 13],
 * row-major, at offset[i] doubles of `blocks` (offset[S] = total), its first row at row row0[i] of the group, its local column c
 * at global column gel_jac_fd_block_cols(phase)[c] (local layout [mass n+1 | position 3(n+1) | velocity 3(n+1) | quaternion
 * 4(n+1) | u 2n | t0 tf]).  6 x 64, velocity rows: 7.8 MB instead of 46.7 MB across PCIe. */
int gel_jac_fd_block_dims(const gel_problem* p, int32_t group, int64_t* rows /* [S] or NULL */, int64_t* cols /* [S] or NULL */,
                          int64_t* row0 /* [S] or NULL */, int64_t* offset /* [S + 1] or NULL */);
int gel_jac_fd_block_cols(const gel_problem* p, int32_t phase, int32_t* cols /* [13 n + 13] */);
int gel_jac_fd_blocks(gel_problem* p, int32_t group, const double* x, double* blocks /* [offset[S]] */);
/* Device-resident form: x and the result stay in HBM (blocks = 0: dense [num_rows[group]][num_vars]; 1: the blocks), launches
 * only, on `stream` (NULL = the handle's); NaN / Inf is reported by the next gel_sync.  One call in flight per handle (the
 * perturbed vectors and their residuals live in the handle). */
int gel_jac_fd_device(gel_problem* p, int32_t group, const double* d_x, double* d_J, int32_t blocks, void* stream);

/* ---- aero path constraints (replace lib/con_aero.py:90-252 inequality_max_alpha /
 *      _q / _qalpha, :254-309 inequality_length_*, :311-756 inequality_jac_max_*).
 *      kind 0 = AOA_max, 1 = dynamic_pressure_max, 2 = Q_alpha_max.  A spec = one entry of
 *      condition[...]: the constrained phase (increasing, < num_sections - 1), range "all" (every state node,
 *      n + 1 rows) or "initial" (1 row), and limit = units[3] (value*pi/180 for kinds 0 and 2, value for 1).
 *      con [B][nrows] = 1 - f/limit.  jac_vals [B][sum nnz4]: the position | velocity | quaternion | t
 *      blocks of the reference's COO values (already negated, con_aero.py:443-463), in its emission order;
 *      gel_aero_pattern gives the matching rows / cols per block (var 0..3). ---- */
int gel_aero_configure(gel_problem* p, int32_t kind, int32_t nspec, const int32_t* phase, const int32_t* range_all,
                       const double* limit);
int gel_aero_dims(const gel_problem* p, int32_t kind, int32_t* nrows, int64_t* nnz4 /* [4] */);
int gel_aero_pattern(const gel_problem* p, int32_t kind, int32_t var, int32_t* rows, int32_t* cols);
int gel_eval_aero(gel_problem* p, int32_t kind, int32_t B, const double* x, double* con, double* jac_vals /* or NULL */);
/* all three kinds in ONE launch (a state node constrained by several kinds runs the air-velocity chain once): con[kind] /
 * jac[kind] as above, NULL = not wanted (jac may be NULL altogether).  Host buffers, or device buffers with the inputs
 * already resident (asynchronous on `stream`; status through gel_sync). */
int gel_eval_aero_all(gel_problem* p, int32_t B, const double* x, double* const* con /* [3] */, double* const* jac /* [3] or NULL */);
int gel_eval_aero_all_device(gel_problem* p, int32_t B, const double* d_x, double* const* d_con /* [3] */,
                             double* const* d_jac /* [3] or NULL */, void* stream);
/* Defect groups AND aero path constraints of a resident batch in one call [r6] -- the hot-path share of objfunc + sens with the aero
 * rows riding on it (lib/con_dynamics.py:216-496 and lib/con_aero.py:89-248,311-371 evaluate the same geodetic -> atmosphere -> wind
 * chain at the same nodes; src/pybind_dynamics.cpp:42-59 / src/wrapper_utils.hpp:89-206).  d_res [B][11 N] and d_jvar [B][V] as
 * gel_eval_batch_device writes them; d_aero [B][width]: ONE record per decision vector in two parts, each
 *   [con alpha | con q | con q-alpha | jac alpha | jac q | jac q-alpha]
 * (part B laid out like gel_eval_aero_all's arrays for its rows, part A spec-major): part A = state nodes 1 .. n of the aerodynamic phases' "all nodes"
 * specs (the rows a lane of the fused kernel has: a spec's row of a column is n doubles -- whole 64-byte lines per store), part
 * B = every other row (state node 0 of a phase, phases without aerodynamics, "initial" specs).  gel_aero_record_layout: width and
 * the twelve section offsets (off_con / off_jac [2][3]: part, kind; every section on a multiple of eight doubles);
 * gel_aero_record_map: the record index of every entry of gel_eval_aero_all's arrays (var = -1: the constraint vector; 0..3: the
 * position / velocity / quaternion / t block in gel_aero_pattern's order) -- the gather a consumer applies, like gel_full_source
 * for the compact Jacobian values; index -1 = an exact zero that is not stored (the t0 / tf columns of part A: the air-relative
 * velocity does not depend on the Earth angle; problems created with GEL_FLAG_FD_RECOMPUTE run those sweeps and store them).
 * Where the launch takes the throughput form with one decision vector per wavefront (not: a handful of vectors, meshes of phases
 * of at most 32 nodes, GEL_FLAG_FD_RECOMPUTE), the lanes of an aerodynamic phase write part A themselves, from the centre
 * evaluation and the position sweeps they run anyway; otherwise -- and with GEL_AERO_FUSED=0 in the environment -- aero_kernel
 * writes it in a launch of its own.  Part B is always a small second launch.  Every value is the same bit for bit as
 * gel_eval_batch_device's and gel_eval_aero_all_device's either way.  Asynchronous on `stream`; status through gel_sync. */
int gel_aero_record_layout(const gel_problem* p, int64_t* width, int64_t* off_con /* [2][3] */, int64_t* off_jac /* [2][3] */);
int gel_aero_record_map(const gel_problem* p, int32_t kind, int32_t var, int64_t* idx);
int gel_eval_batch_aero_device(gel_problem* p, int32_t B, const double* d_x, double* d_res, double* d_jvar, double* d_aero,
                               void* stream);
/* which form aero_kernel's launcher takes for B vectors, from the function the launcher itself decides by (like gel_launch_info; works
 * on GEL_DEVICE_NONE handles).  records = 0: the dense arrays of gel_eval_aero_all_device; 1: part A of the records of
 * gel_eval_batch_aero_device where aero_kernel writes it (GEL_AERO_FUSED=0, GEL_FLAG_FD_RECOMPUTE, GEL_FLAG_EXACT_AERO_JAC, batches the
 * fused form does not take).  info = {1 flat (vector, node) mapping with 32-bit byte offsets / 0 one tile per vector, number of runs
 * the batch is launched in, vectors per full-length run, bytes that one run's gradient values of the largest kind span}.  A last,
 * shorter run decides its own form: ask again with its length. */
int gel_aero_launch_info(const gel_problem* p, int32_t B, int32_t records, int64_t* info /* [4] */);

/* ---- knot / terminal / user rows.
 *  Linear rows: value = (coef0 * x[idx0] + coef1 * x[idx1]) + c0 (idx1 < 0: one term) over the packed decision vector --
 *    what equality_init, equality_time, inequality_time and equality_knot_LGR compute
 *    (lib/con_init_terminal_knot.py:39-52,118-141,174-252,422-436); with coefficients +-1 it rounds like the
 *    reference's (a - b) - c.  Their Jacobians are these coefficients: constant COO blocks the caller lays out.
 *  Node-function rows: a function f of ONE knot state (r = position * unit_position, v = velocity * unit_velocity of state
 *    node `node`; for fn >= 9 also the knot time t = x_t[tcol] * unit_t) and its forward difference over the seven
 *    columns the row can see (position xyz, velocity xyz of that node, then the knot time), formed in the kernel.
 *      mode & 3: value = f / p[0] - p[1] (0) or (f - p[1]) / p[0] (1); mode & 8: negated ("max" rows).
 *      mode & 4 clear: difference of the value itself, (value(x + dx e_c) - value(x)) / dx -- what lib/jac_fd.py and
 *        equality_jac_6DoF_LGR_terminal do; set: ((f(x + dx e_c) - f(x)) / dx) / p[0] (negated with mode & 8) -- what
 *        lib/con_waypoint.py does.
 *      fn 0 orbit energy, 1 angular momentum, 2 inclination [rad]  -> equality_6DoF_LGR_terminal and its Jacobian
 *        (lib/con_init_terminal_knot.py:329-405, src/wrapper_coordinate.hpp:222-250);
 *      fn 3 a, 4 e, 5 a(1-e), 6 a(1+e) of the orbital elements (src/Coordinate.cpp:197-245), 7 |r|, 8 |v|
 *        -> the shipped user constraint example/user_constraints.py:120-139 (fn 5, p = {6378137, 1}), whose generic
 *        lib/jac_fd.py:29-62 loop perturbs every column of x and gets an exact zero for all but these;
 *      fn 9 / 10 / 11 geodetic latitude / longitude [deg] / altitude [m] at the knot time -> equality_posLLH,
 *        inequality_posLLH (lib/con_waypoint.py:507-560,717-784); fn 12 / 13 latitude / longitude [deg] of the
 *        instantaneous impact point (FAA algorithm, lib/IIP.py:30-135) -> equality_IIP, inequality_IIP (:164-207,330-381);
 *        fn 14 sine of the elevation above an antenna's horizon, p[2..4] = antenna ECEF position, p[5..7] = its local
 *        vertical -> inequality_antenna (:45-51,70-105); fn 15 downrange [m]: Vincenty distance (lib/downrange.py:32-111)
 *        from the launch point p[2] = latitude, p[3] = longitude [deg] to the position's geodetic latitude / longitude
 *        -> the "downrange" rows of equality_posLLH / inequality_posLLH (:531-534,551-554,742,771-778) and their gradient
 *        (downrange_gradient, :583-607).
 *  con [B][nlin + nfn] (linear rows first); jfn [B][nfn][7]. ---- */
typedef struct { int32_t idx0, idx1; double coef0, coef1, c0; } gel_linear_row;
typedef struct { int32_t fn, node, tcol, mode; double p[8]; } gel_nodefn_row;
int gel_rows_configure(gel_problem* p, int32_t nlin, const gel_linear_row* lin, int32_t nfn, const gel_nodefn_row* fn);
int gel_rows_dims(const gel_problem* p, int32_t* nlin, int32_t* nfn);
int gel_rows_eval(gel_problem* p, int32_t B, const double* x, double* con, double* jfn /* or NULL */);
int gel_rows_eval_device(gel_problem* p, int32_t B, const double* d_x, double* d_con, double* d_jfn /* or NULL */, void* stream);

/* ---- collocation error estimate per section (the LGR mesh-error estimate of Garg et al. 2009 / GPOPS-II's ph method; DESIGN.md
 *      3.9): is the trajectory accurate BETWEEN the nodes?  For phase s of n nodes, on its own tau (generated or desc.tau), with
 *      the flipped LGR points sigma_1 .. sigma_{n+1} of n + 1 (sigma_{n+1} = +1, sigma_0 = -1):
 *        X~(sigma_l) = sum_i Lx[l][i] X_i   (Lagrange basis on tau_x = [-1, tau], the n + 1 state nodes xa .. xa + n; X~(sigma_0) = X_0)
 *        U~(sigma_l) = sum_j Lu[l][j] U_j   (Lagrange basis on tau, the n collocation nodes' u)
 *        F_l = the right-hand side the phase's DEFECT ROWS impose, at (X~, U~, t(sigma_l) = sigma_l (tf - to)/2 + (tf + to)/2
 *              normalised, as PSparams.time_nodes): mass -massflow/unit_mass with the engine on, else 0; position
 *              X~_vel unit_v/unit_p; velocity dynamics_velocity (reference_area != 0) or _NoAir, / unit_v; quaternion
 *              dynamics_quaternion, or 0 for a held attitude
 *        X^(sigma_j) = X_0 + S sum_l I[j][l] F_l,  S = (tf - to) unit_t / 2,  I = (D^[:, 1:])^-1, D^ = gel_lgr_diffmat(n + 1)
 *        e_{j,c} = |X^_c(sigma_j) - X~_c(sigma_j)| / (1 + max_{l=0..n+1} |X~_c(sigma_l)|)
 *      over the 11 state components c (x's order: mass, position 3, velocity 3, quaternion 4).  The matrices are built at
 *      gel_problem_create in extended precision (host-only handles included); phases of more than 511 nodes have none and the
 *      gel_mesh_* calls but gel_mesh_dims refuse such a handle.  The flags of the handle do not change the estimate. ---- */
/* npts = sum over phases of (n_s + 1): the test points, in phase order (the rows of diff) */
int gel_mesh_dims(const gel_problem* p, int32_t* npts);
/* phase's fine grid and matrices, row-major (P = n + 1); any pointer may be NULL */
int gel_mesh_matrices(const gel_problem* p, int32_t phase, double* sigma /* [P] */, double* Lx /* [P][n+1] */,
                      double* Lu /* [P][n] */, double* I /* [P][P] */);
/* B decision vectors x [B][num_vars] -> err [B][S][4]: max of e over the test points and over the components of each group
 * (mass, position, velocity, quaternion); diff (NULL: not wanted) [B][npts][11]: the signed X^ - X~ at every test point.  Returns
 * GEL_NONFINITE when an output is NaN / Inf (the other vectors' outputs stay valid).  Host buffers; one device launch. */
int gel_mesh_error(gel_problem* p, int32_t B, const double* x, double* err, double* diff /* or NULL */);
/* the same on device buffers, asynchronous on `stream` (NULL = the handle's); status through gel_sync */
int gel_mesh_error_device(gel_problem* p, int32_t B, const double* d_x, double* d_err, double* d_diff /* or NULL */, void* stream);

/* ---- batched Jacobian products from the compact values: y_b = J(x_b) v_b and g_b = J(x_b)^T lambda_b for the
 *      four defect groups (the 13 COO blocks), where J(x_b) is exactly the matrix that gel_pattern_all + gel_const_values +
 *      gel_full_source applied to jvar[b] define -- whatever the handle's flags put into jvar.  The full value array is never
 *      formed.  Rows of y / lambda in the residual order [mass N | pos 3N | vel 3N | quat 4N]; columns of v / g in the packed
 *      decision-vector order.  Every element of y and g is written by every call (a column without an entry gets 0.0).  A vector's
 *      results depend neither on its neighbours in the batch nor on B, and are bit-identical run to run (no floating-point
 *      atomics; every sum has a fixed order).  The operator tables are built by gel_problem_create from the same pattern walk
 *      as the gather map (host-only handles included). ---- */
/* device buffers, asynchronous on `stream` (NULL = the handle's); status through gel_sync: GEL_NONFINITE when some output is
 * NaN / Inf (the other vectors' outputs stay valid).  gel_jac_rmatvec_device keeps per-phase partial sums of the time columns
 * in a workspace of the handle: calls on one handle must not overlap on different streams. */
int gel_jac_matvec_device(gel_problem* p, int32_t B, const double* d_jvar /* [B][V] */, const double* d_v /* [B][num_vars] */,
                          double* d_y /* [B][11N] */, void* stream);
int gel_jac_rmatvec_device(gel_problem* p, int32_t B, const double* d_jvar /* [B][V] */, const double* d_lam /* [B][11N] */,
                           double* d_g /* [B][num_vars] */, void* stream);
/* the same on host buffers (copy in, one launch, copy out, one synchronise); returns GEL_OK or GEL_NONFINITE */
int gel_jac_matvec(gel_problem* p, int32_t B, const double* jvar, const double* v, double* y);
int gel_jac_rmatvec(gel_problem* p, int32_t B, const double* jvar, const double* lam, double* g);
/* plain C++ on the host from the SAME tables (works on GEL_DEVICE_NONE handles): transpose = 0: in = v, out = y; else in = lambda,
 * out = g.  Returns GEL_OK or GEL_NONFINITE. */
int gel_jac_products_host(const gel_problem* p, int32_t B, const double* jvar, const double* in, double* out, int32_t transpose);
/* info [4]: non-zero constant entries, variable entries, largest non-zero count of a row, of a column (variable entries count
 * as non-zero) */
int gel_jac_products_info(const gel_problem* p, int64_t* info);
/* what a product launch will use, as gel_jac_*_device decide it: info = {vectors per workgroup of J v, lanes per workgroup, the same
 * two for J^T lambda}.  GEL_JPROD_VB (read per call) and GEL_JPROD_THREADS (read when the handle is created) are honoured; works on
 * GEL_DEVICE_NONE handles.  (An entry point of its own: gel_jac_products_info's callers hold four values.) */
int gel_jac_products_launch_info(const gel_problem* p, int32_t* info /* [4] */);

/* ---- batched products with K(x_b), the Jacobian of EVERY ROW THAT IS NOT A DEFECT ROW: y_b = K v_b and
 *      g_b = K^T lambda_b.  The values are read where the launches that produce them leave them -- jfn [B][nfn][7] of
 *      gel_rows_eval_device, and EITHER the dense arrays jac[kind] of gel_eval_aero_all_device OR the records of
 *      gel_eval_batch_aero_device; a gathered or full form is never built.
 *      Definition of K.  Rows [linear nlin | node-function nfn | alpha rows | q rows | q-alpha rows], R = nlin + nfn + sum of
 *      the kinds' nrows: gel_rows_eval's con followed by gel_eval_aero_all's three con arrays.  Columns: the packed decision vector.
 *        linear row r:        (r, idx0) = coef0; if idx1 >= 0, (r, idx1) = coef1.
 *        node-function row r (global row nlin + r): jfn[r][0..2] at the position columns M + 3 node + c, jfn[r][3..5] at the
 *                             velocity columns 4M + 3 node + c, jfn[r][6] at column 11M + 2N + tcol ONLY IF tcol >= 0; with
 *                             tcol < 0 jfn[r][6] is not read (a NaN there reaches no output).
 *        aero rows of kind k: exactly the triplets of gel_aero_pattern(kind, var), var 0..3, the column shifted by the variable's
 *                             offset (M, 4M, 7M, 11M + 2N); the value is the matching element of jac[kind] (dense form) or
 *                             record[gel_aero_record_map(kind, var)[e]] (record form).
 *        structural zeros:    an entry whose record-map index is -1 (the t0 / tf columns of part A on handles without
 *                             GEL_FLAG_FD_RECOMPUTE) is NOT an entry of K, in either source form: the dense value there is
 *                             not read, and both forms give the same bits.
 *        shared cells:        where several entries share one (row, col), the cell is their sum.
 *      The handle's flags (8, 32, 64, 128) change the values the caller passes in, not the operator.
 *      Summation order (part of the contract).  Every output is ONE fma chain acc = fma(value, in, acc) from +0.0 over its entries:
 *      a row of K v in the order of its definition above (linear: idx0, idx1; node-function: jfn column 0 .. 6; aero: var 0, 1, 2,
 *      3, inside a var the order of gel_aero_pattern -- for t: t0, then tf); a column of K^T lambda by ascending row, the entries
 *      of one row in that row's own order.  The order depends on the handle's configuration alone: not on B, not on the vector's
 *      position in the batch, not on the source form, not on any launch parameter; the host form runs the same chains and gives
 *      the same bits.  No floating-point atomics.  A column without an entry gets +0.0.
 *      The tables are rebuilt whenever gel_rows_configure or gel_aero_configure succeeds (host-only handles included) and swapped in
 *      with the tables of that call; a configure call that fails leaves the old operator in place.
 *      Arguments: exactly one of aero_jac and aero_record is non-NULL when any aero kind has rows, both are NULL when none has;
 *      inside aero_jac a kind without rows may be NULL; jfn may be NULL only when nfn = 0; R = 0 (nothing configured), B < 1 or a
 *      NULL input / output return GEL_ERR_ARG.
 *      Streams: the device calls take no stream argument; like gel_interp_resident and gel_propagate_device they enqueue on the
 *      handle's own stream, which is a blocking stream and so orders itself against the null stream.  A caller working on a
 *      NON-BLOCKING stream must have finished writing the inputs before the call and must gel_sync(p, NULL) before it consumes the
 *      outputs.  (A `void* stream` parameter would need a case in the caller-stream case table, tests/stream_cases.py, which the
 *      guard tests/test_caller_stream_cpu.py holds against this header; it belongs with a change that extends that table.)
 *      Status: a lane that stores a non-finite value raises the handle's flag (gel_sync); a NaN among one vector's inputs stays in
 *      that vector's outputs. ---- */
/* info [9]: R, nlin, nfn, alpha rows, q rows, q-alpha rows, entries of K, largest entry count of a row, of a column (nine values:
 * R itself and the eight counts behind it).  Works on GEL_DEVICE_NONE handles. */
int gel_con_products_dims(const gel_problem* p, int64_t* info /* [9] */);
/* device buffers, asynchronous on the handle's own stream: d_y [B][R] */
int gel_con_matvec_device(gel_problem* p, int32_t B, const double* d_jfn, const double* const* d_aero_jac /* [3] or NULL */,
                          const double* d_aero_record /* or NULL */, const double* d_v /* [B][num_vars] */, double* d_y);
/* d_g [B][num_vars].  accumulate = 0: every element of g is written; accumulate = 1: g = fl(g_in + s), s exactly the value the call
 * writes with accumulate = 0 -- gel_jac_rmatvec_device followed by this call gives J^T lambda_defect + K^T lambda_other in one
 * buffer, bit for bit the sum of the two separate results. */
int gel_con_rmatvec_device(gel_problem* p, int32_t B, const double* d_jfn, const double* const* d_aero_jac /* [3] or NULL */,
                           const double* d_aero_record /* or NULL */, const double* d_lam /* [B][R] */, double* d_g, int32_t accumulate);
/* the same on host buffers (copy in, one launch, copy out, one synchronise); return GEL_OK or GEL_NONFINITE */
int gel_con_matvec(gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                   const double* v, double* y);
int gel_con_rmatvec(gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                    const double* lam, double* g, int32_t accumulate);
/* plain C++ on the host from the SAME tables in the same order (works on GEL_DEVICE_NONE handles): transpose = 0: in = v, out = y;
 * else in = lambda, out = g.  Returns GEL_OK or GEL_NONFINITE. */
int gel_con_products_host(const gel_problem* p, int32_t B, const double* jfn, const double* const* aero_jac, const double* aero_record,
                          const double* in, double* out, int32_t transpose, int32_t accumulate);

/* ---- batched spectral interpolation: dense output and mesh transfer.  Per phase the collocation solution is a
 *      polynomial: degree n in the 11 state components on the support [-1, tau_1 .. tau_n] (the n + 1 state nodes), degree n - 1
 *      in the 2 controls on tau_1 .. tau_n.  A PLAN holds, for every phase of its source handle (on the handle's own tau, generated
 *      or desc.tau), the matrices that evaluate this polynomial at the plan's points,
 *        Wx[l][i] = the Lagrange basis on [-1, tau_1 .. tau_n] at point l,   Wu[l][j] = the basis on tau_1 .. tau_n at point l,
 *      built at plan creation in extended precision with barycentric weights and rounded once (nothing is built at
 *      gel_problem_create).  A point that equals a support node as an fp64 number is a COPY: copy_x[l] / copy_u[l] holds the
 *      support index (else -1), its row is the unit row, and the value is copied, not multiplied -- bit-exact: a signed zero keeps
 *      its sign and a NaN elsewhere in the phase does not reach it.  With generated nodes tau_n = +1 and the state support's -1
 *      are exact, so every section's first and last state node is a copy between any two meshes (the knot states the linear
 *      continuity rows read keep their bits), and a transfer between equal meshes is a bitwise copy.
 *      Every other output is ONE fma chain over the support index in ascending order, starting from +0.0, on the device and in
 *      gel_interp_host alike: both give the same bits, and a vector's result depends neither on B, nor on its position in the
 *      batch, nor on the number of vectors a workgroup carries.
 *      Table mode (mode 0): out [B][npts][14], rows in phase order, points in the order given; column 0 = the normalised time
 *      sigma (tf - to)/2 + (tf + to)/2, columns 1..11 = the states (mass, position 3, velocity 3, quaternion 4), columns 12..13
 *      = the controls, all in x's normalised units.  A control sampled below tau_1 is the control polynomial EXTRAPOLATED (the
 *      controls have no node at -1).
 *      Transfer mode (mode 1): the points are the destination handle's own nodes (states at [-1, tau^d], controls at tau^d);
 *      out [B][dst num_vars] is the destination's packed decision vector, t copied bit for bit.  src and dst must have the same
 *      number of phases.
 *      Every element of out is written by every call.  GEL_INTERP_UNIT_QUAT: at rows that are not copies q is replaced by
 *      q / sqrt(q . q) (the dot product one fma chain over components 0 .. 3); without the flag the map is purely linear.
 *      A non-finite output raises the SOURCE handle's status: gel_interp and gel_interp_host return GEL_NONFINITE, the resident
 *      form reports it through gel_sync(src, NULL); the other vectors' outputs stay valid.
 *      Streams: gel_interp_resident takes no stream argument; it enqueues on the source handle's own stream, which is a blocking
 *      stream and so orders itself against the null stream.  A caller working on a NON-BLOCKING stream must gel_sync(src, NULL)
 *      before it consumes the output (and must have finished writing d_x before the call).
 *      Lifetime: a plan is destroyed BEFORE its source handle; the destination handle of a transfer plan may be a host-only handle
 *      and may be destroyed right after the plan is created.  A plan on a device handle refuses (GEL_ERR_ARG) a phase whose
 *      staged slice, 13 n + 11 doubles, does not fit a workgroup's 64 KB of LDS (n > 629); gel_interp_host on a host-only
 *      handle has no such limit.  B = 0 and npts[s] = 0 are valid. ---- */
typedef struct gel_interp_plan gel_interp_plan; /* opaque */
#define GEL_INTERP_UNIT_QUAT 1
/* table mode: npts[s] points per phase (0 allowed), pts concatenated, each finite and in [-1, 1] */
int gel_interp_plan_create(gel_problem* src, const int32_t* npts /* [S] */, const double* pts, int32_t flags, gel_interp_plan** out);
/* transfer mode: the points are dst's own nodes; dst may be a host-only handle and may be destroyed afterwards */
int gel_interp_plan_create_transfer(gel_problem* src, const gel_problem* dst, int32_t flags, gel_interp_plan** out);
int gel_interp_plan_destroy(gel_interp_plan* plan);
/* info [6]: S, mode (0 table, 1 transfer), state rows (table: the points; transfer: the destination's M), doubles per output
 * vector, src num_vars, vectors per workgroup a launch will use NOW (the largest of 4, 2, 1 whose staged slice fits; GEL_INTERP_VB
 * = 1 / 2 / 4 in the environment, read per call, overrides it where it fits) */
int gel_interp_plan_info(const gel_interp_plan* plan, int64_t* info /* [6] */);
/* row-major; P = Pu = npts[phase] (table), P = n_d + 1 and Pu = n_d (transfer); any pointer may be NULL */
int gel_interp_matrices(const gel_interp_plan* plan, int32_t phase, double* Wx /* [P][n+1] */, double* Wu /* [Pu][n] */,
                        int32_t* copy_x /* [P] */, int32_t* copy_u /* [Pu] */);
int gel_interp(gel_interp_plan* plan, int32_t B, const double* x, double* out);              /* host buffers, one launch, synchronised */
int gel_interp_resident(gel_interp_plan* plan, int32_t B, const double* d_x, double* d_out); /* device buffers, asynchronous */
int gel_interp_host(const gel_interp_plan* plan, int32_t B, const double* x, double* out);   /* plain C++, works for GEL_DEVICE_NONE */

/* ---- batched explicit propagation of the sections with classical RK4: the shooting check.  Take the controls
 *      of a decision vector, integrate the equations of motion explicitly from a section's first state and see whether the
 *      trajectory arrives where the collocated states say -- a check that uses neither D nor I.
 *      Phase s of n nodes, support tau_x = [-1, tau_1 .. tau_n], S = (tf - to) unit_t / 2, k = steps[s] >= 1:
 *      Steps: every node interval [tau_x_j, tau_x_{j+1}] is cut into k equal RK4 steps h_j = (tau_x_{j+1} - tau_x_j) / k (fp64).
 *      The phase has Pp = 2 k n + 1 STAGE POINTS; point 2 (k j + i) + m, m = 0, 1, 2, is tau_x_j + (tau_x_{j+1} - tau_x_j)
 *      (2 i + m) / (2 k), formed in extended precision and rounded once; a point that falls on a node is the node's fp64 value.
 *      Right-hand side F(sigma, X, U): exactly the one gel_mesh_error evaluates (mass -massflow/unit_mass with the engine on, else
 *      0; position X_vel unit_v/unit_p; velocity dynamics_velocity or _NoAir by reference_area, at the normalised time sigma
 *      (tf - to)/2 + (tf + to)/2; quaternion dynamics_quaternion, or 0 for a held attitude).  Quaternions are never renormalised.
 *      Controls: U(sigma) = the control polynomial on tau_1 .. tau_n sampled at the stage points with Wu [Pp][n], built as
 *      gel_interp_plan_create builds its Wu (the same bits), each sample ONE fma chain over the node index in ascending order from
 *      +0.0; a stage point that is a collocation node is a copy (copy_u); below tau_1 the polynomial is extrapolated.
 *      Step (y at the step's first stage point p; every operation rounds once, fma where written):
 *        Sh = S h_j;  k1 = F(p, y);  k2 = F(p + 1, fma(Sh/2, k1, y));  k3 = F(p + 1, fma(Sh/2, k2, y));  k4 = F(p + 2, fma(Sh, k3, y))
 *        a = fma(2, k2, k1);  a = fma(2, k3, a);  a = fma(1, k4, a);  y <- fma(Sh / 6, a, y)
 *      Restart: by default (section mode) y starts at X_0 of the section and runs to its last node; with GEL_PROP_RESTART_NODE every
 *      node interval starts from the collocated X_j (the local defect: WHERE a section is bad).  The first interval is the same
 *      computation in both modes: the same bits.
 *      Chain (GEL_PROP_CHAIN, excludes GEL_PROP_RESTART_NODE): the flight.  One integration per vector from lift-off to the last
 *      node, the phases in order; to and tf of every phase come from the vector's own x, as in the other modes.  Phase 0 starts at
 *      its X_0, bit for bit.  Across the knot into phase s + 1, per component c: jump = x_c(first node of s + 1) - x_c(last node of
 *      s) (one subtraction); the start value is y_c itself where jump == 0, else y_c + jump (one addition) -- a continuous knot
 *      carries the bits, a stage drop carries the collocated mass jump without reading the row table.  The carried state is what y
 *      holds at node xa of phase s + 1.  err is then the ACCUMULATED flight error per section; its last row is the terminal miss.
 *      Dispersions (gel_propagate_dispersed*): disp [B][S][GEL_PROP_NDISP] or NULL, valid in all three modes; each factor f is
 *      used as ONE fp64 product, formed once per (vector, phase):
 *        index 0  thrust          thrust f: the vacuum thrust; the nozzle term nozzle_area P is untouched
 *        index 1  mass flow       (-massflow / unit_mass) f
 *        index 2  reference area  reference_area f (to the dynamics the same thing as a CA or density scale)
 *        index 3  wind            wn f, we f: the two interpolated wind components (the tables are shared by the vectors of a
 *                                 workgroup), before the rotation into ECI
 *      dynamics_velocity against _NoAir is still decided by the HANDLE's reference_area.  A factor of exactly 1.0 changes no bit,
 *      and gel_propagate* is gel_propagate_dispersed* with NULL.  A non-finite factor makes that vector's outputs non-finite and
 *      raises the status like any NaN; the other vectors are unaffected.
 *      Outputs: y [B][11 M], laid out like the state part of x (mass M | position 3M | velocity 3M | quaternion 4M): the propagated
 *      state at every state node; node xa of each phase is X_0 copied bit for bit.  err (optional) [B][S][4] in gel_mesh_error's
 *      normalisation: max_{i=1..n} |y_c(i) - x_c(i)| / (1 + max_{i=0..n} |x_c(i)|), then the maximum over each group's components
 *      (mass, position, velocity, quaternion); a NaN is kept.  Every element is written by every call.  A non-finite output raises
 *      the source handle's status (GEL_NONFINITE from gel_propagate, through gel_sync for the device form); the other vectors'
 *      outputs stay valid.  A vector's result depends neither on B, nor on its position in the batch, nor on anything another
 *      vector holds, nor on the slab size.
 *      Refusals (GEL_ERR_ARG): steps[s] < 1; steps[s] n_s > 2^20, and for a chain plan sum_s steps[s] n_s > 2^20 (no lane runs
 *      longer than that many steps: a launch always ends); both mode flags at once;
 *      control matrices of more than 2^27 doubles in all (sum of Pp n); on a device handle a free-attitude phase of more than 1024
 *      nodes (its controls are staged in a workgroup's LDS) and more than 2^20 stage points of free-attitude phases in all (the
 *      control samples of 64 vectors, 16 bytes per stage point, must fit the 1 GB workspace).
 *      The plan owns every buffer it needs: its tables, the control samples' workspace [stage point][2][vector] (16 bytes per
 *      stage point of a free-attitude phase and vector, capped at 1 GB: a larger batch is walked in slabs of vectors on the stream)
 *      and the working set of gel_propagate.  A plan is destroyed BEFORE
 *      its source handle.  B = 0 is valid.  There is no host form: the evaluation calls refuse a GEL_DEVICE_NONE handle. ---- */
typedef struct gel_prop_plan gel_prop_plan; /* opaque */
#define GEL_PROP_RESTART_NODE 1
#define GEL_PROP_CHAIN 2
#define GEL_PROP_NDISP 4
int gel_prop_plan_create(gel_problem* src, const int32_t* steps /* [S] */, int32_t flags, gel_prop_plan** out);
int gel_prop_plan_destroy(gel_prop_plan* plan);
/* info [6]: S, flags, stage points in total (sum of Pp), RK4 steps of the longest lane (max k n, max k with
 * GEL_PROP_RESTART_NODE, sum of k n with GEL_PROP_CHAIN), workspace bytes per vector, vectors per slab a call will use NOW (the most the workspace cap holds, a
 * multiple of 64; GEL_PROP_SLAB in the environment, read per call and rounded up to a multiple of 64, overrides it where it fits) */
int gel_prop_plan_info(const gel_prop_plan* plan, int64_t* info /* [6] */);
/* row-major, Pp = 2 steps[phase] n + 1; any pointer may be NULL; works on GEL_DEVICE_NONE handles */
int gel_prop_matrices(const gel_prop_plan* plan, int32_t phase, double* pts /* [Pp] */, double* Wu /* [Pp][n] */,
                      int32_t* copy_u /* [Pp] */);
/* host buffers, synchronised; returns GEL_OK or GEL_NONFINITE; err may be NULL */
int gel_propagate(gel_prop_plan* plan, int32_t B, const double* x, double* y, double* err);
/* device buffers, asynchronous; like gel_interp_resident it takes no stream argument: everything is enqueued on the source
 * handle's own stream, which is a blocking stream and so orders itself against the null stream; status through
 * gel_sync(src, NULL).  A caller working on a NON-BLOCKING stream must have finished writing d_x before the call and must
 * gel_sync(src, NULL) before it consumes the outputs. */
int gel_propagate_device(gel_prop_plan* plan, int32_t B, const double* d_x, double* d_y, double* d_err /* or NULL */);
/* the same pair with per-vector, per-phase factors disp [B][S][GEL_PROP_NDISP] (or NULL: exactly the pair above) */
int gel_propagate_dispersed(gel_prop_plan* plan, int32_t B, const double* x, const double* disp /* or NULL */, double* y, double* err);
int gel_propagate_dispersed_device(gel_prop_plan* plan, int32_t B, const double* d_x, const double* d_disp /* or NULL */, double* d_y,
                                   double* d_err /* or NULL */);

/* ---- tangent-linear propagation: exact flight sensitivities.  gel_propagate_tangent* returns the y of
 *      gel_propagate_dispersed* on the same plan, x and disp -- bit for bit -- and dy [B][P][11 M]: for every vector b and direction
 *      p the derivative of that discrete RK4 map (the step above, as it is coded) along a seed (dx, ddisp).  All three plan modes.
 *      Seeds: dx is laid out like a decision vector [nvars]; only what the value call reads from x is read from dx: the state row
 *      a segment starts from (chain: phase 0's X_0; section mode: every section's first node; node mode: every node), in chain
 *      mode both state rows of every knot (djump = dx(first node of s + 1) - dx(last node of s)), the controls of the
 *      free-attitude phases and the knot times.  ddisp [S][GEL_PROP_NDISP] is the direction in the four factors (disp == NULL:
 *      the factors are one).  Either seed may be NULL (zero), not both.  shared = 0: per (vector, direction), dx [B][P][nvars] and
 *      ddisp [B][P][S][4]; shared = 1: one set [P][...] serves every vector (its control directions are sampled once).
 *      Tangent of a step, term by term in this order (F, dF: the previous stage's):  dS = (dtf - dto) unit_t / 2, dSh = dS h_j;
 *        dyt = fma(da, F, fma(a, dF, dy)) for the stages with a = Sh/2, Sh/2, Sh and da = dSh/2, dSh/2, dSh (stage 1: dyt = dy);
 *        dF = J dyt + dF/du dU + dF/dfactors df, dU the control direction sampled like U (Wu du, a node copied), the factors
 *        as the value applies them (thrust df0, mf_um df1, area df2, d(wn fw) = wn dfw + fw dwn);
 *        dacc = fma(w, dF, dacc), w = 2, 2, 1 (stage 1: dacc = dF);  dy <- fma(dSh / 6, acc, fma(Sh / 6, dacc, dy)).
 *      J and the partials are the hand-written fp64 tangents of GEL_FLAG_EXACT_DEFECT_JAC with their conventions at kinks (the
 *      derivative of the branch the value took); the explicit time dependence of F (the Earth angle, read on the polar axis only)
 *      has tangent zero, as in that flag's t columns.  Knot (chain): dy where djump == 0, else dy + djump.  Quaternions are not
 *      renormalised; a hold phase has zero quaternion rows, an engine-off phase a zero mass row.  The tangent is linear in the
 *      seed with no additive constant: a zero seed gives dy == 0, a seed times 2^k gives dy times 2^k bit for bit.  Direction p's
 *      bits depend neither on P, nor on B, nor on the slab size.  There is no err output.  Under a wind ensemble:
 *      gel_propagate_tangent_ensemble* below.
 *      Status: a non-finite y or dy raises the source handle's status as gel_propagate* does; the other (vector, direction)
 *      slices stay valid.  Refusals (GEL_ERR_ARG): P < 1; B P > 2^31 - 1; both seeds NULL; shared not 0 or 1; a host-only handle;
 *      seeds whose control samples for 64 vectors do not fit the plan's 1 GB workspace.  B = 0 succeeds and touches nothing.
 *      The workspace holds 1 + P sample sets per vector (shared: 1 per vector and P in all); a larger batch is walked in slabs,
 *      GEL_PROP_SLAB (vectors) as above.  The device form takes no stream argument: it enqueues on the handle's own stream and
 *      reports through gel_sync(src, NULL), like gel_propagate_device. ---- */
int gel_propagate_tangent(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp /* or NULL */,
                          const double* dx /* or NULL */, const double* ddisp /* or NULL */, double* y, double* dy);
int gel_propagate_tangent_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x,
                                 const double* d_disp /* or NULL */, const double* d_dx /* or NULL */, const double* d_ddisp /* or NULL */,
                                 double* d_y, double* d_dy);
/* info [3]: bytes of one sample set (per vector of a slab, and per seed: per lane, or per direction when shared), lanes
 * (vector, direction) per slab a call will use NOW, slabs of a call of B vectors; works on GEL_DEVICE_NONE handles */
int gel_prop_tangent_info(const gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, int64_t* info /* [3] */);

/* ---- adjoint flight: gradients of the flown trajectory in one pass.  Let T = [T_x | T_d] be the linear map
 *      gel_propagate_tangent* applies, dy = T_x dx + T_d ddisp, as it is coded (its conventions at kinks, the zero time tangent of
 *      F, djump, dS = (dtf - dto) unit_t / 2).  gel_propagate_adjoint* returns the y of gel_propagate_dispersed* on the same plan, x
 *      and disp -- bit for bit -- and, for Q functionals per vector given as weights lam on y,
 *        gx [B][Q][nvars] = T_x^T lam        gdisp [B][Q][S][GEL_PROP_NDISP] = T_d^T lam   (gdisp may be NULL: not wanted).
 *      lam is laid out like y: [B][Q][11 M], or with shared = 1 one set [Q][11 M] for every vector.  Any node's rows may carry
 *      weight; a terminal functional is a lam that is zero except in the last node's rows.  Entries of gx for inputs the value call
 *      does not read (state rows that start no segment and lie at no chain knot, a hold phase's controls) are +0.0; every element
 *      of gx and gdisp is written by every call.
 *      Chain (GEL_PROP_CHAIN) and section plans.  GEL_PROP_RESTART_NODE plans are refused: neighbouring node segments share a stage
 *      point, whose control multiplier would need a second accumulation path.  Under a wind ensemble: gel_propagate_adjoint_ensemble* below.
 *      The value flight runs first; its y(node j) is the checkpoint interval j restarts from.  Then every (vector, functional) walks
 *      backwards -- phases S - 1 .. 0 (on a section plan too, where l starts at zero in every phase), intervals n - 1 .. 0, steps
 *      k - 1 .. 0 -- and every step is the transpose of the
 *      tangent's step, term by term in this order (l = the multiplier of the step's end state; F1 .. F3 recomputed with the value's
 *      own lines from the step's start: the node's checkpoint, or an inner checkpoint -- per node interval the k - 1 value steps to
 *      the starts of its later steps are integrated once more and kept per lane):
 *        lacc = (Sh / 6) l;   lF4 = lacc;  lF3 = fma(Sh, lyt4, 2 lacc);  lF2 = fma(Sh/2, lyt3, 2 lacc);  lF1 = fma(Sh/2, lyt2, lacc)
 *        with (lyt_i, lu_i, lfactors_i) = (J^T, (dF/du)^T, (dF/dfactors)^T) lF_i at stage i's point, the same partials as the tangent;
 *        l <- l + (((lyt4 + lyt3) + lyt2) + lyt1);
 *        gS <- fma(h_j, <l, acc> / 6 + <lyt4, F3> + <lyt3, F2> / 2 + <lyt2, F1> / 2, gS)      (l before its update, acc the value's)
 *      lam's rows of a node are added to l where the walk passes the node.  A segment's start row gets l; across a chain knot
 *      gx(first node of s + 1) = l, gx(last node of s) = 0 - l, and l carries on.  The factors' multipliers are summed over a
 *      phase's stages in walk order and multiplied by the handle's thrust, mf_um and area (the wind factor's by 1).  The stage
 *      points' control multipliers are stored once each (a step's end point: stage 4's plus stage 1's of the step after it; its
 *      midpoint: stage 2's + stage 3's) and carried to the nodes by the transposed sampler: gu(node j) = one fma chain over the
 *      stage points in ascending order of Wu[p][j] lu(p), in which a point that IS a node is skipped (the value call copies the
 *      node there) and added to that node's result instead.  Knot times: gt(s) = ((gS(s - 1) - gS(s)) unit_t) / 2, gS(-1) = gS(S) = 0.
 *      No atomic operation anywhere: every output has one writer and the order above.  The result is linear in lam with no additive
 *      constant: lam == 0 gives zeros, lam times 2^k gives the outputs times 2^k bit for bit.  Functional q's bits depend neither on
 *      Q, nor on B, nor on the vector's position in the batch, nor on the slab size, nor on shared.
 *      Status: a non-finite y, gx or gdisp raises the source handle's status as gel_propagate* does; the other (vector, functional)
 *      slices stay valid.  Refusals (GEL_ERR_ARG, decided before a buffer is looked at, the reason in gel_last_error): Q < 1;
 *      B Q > 2^31 - 1; lam == NULL; shared not 0 or 1; a host-only handle; a GEL_PROP_RESTART_NODE plan; a plan whose sum of steps[s] n_s
 *      exceeds 2^20 (one (vector, functional) walks every phase, so a section plan is held to the chain's limit here); a workspace
 *      that does not fit the plan's 1 GB cap for 64 vectors.  B = 0 succeeds and touches nothing.
 *      The workspace holds one sample set per vector and, per (vector, functional), the stage points' control multipliers (as many
 *      bytes again), one double per phase and 88 (max steps[s] - 1) bytes of inner checkpoints; a larger batch is walked in slabs, GEL_PROP_SLAB (vectors) as above.  The device form
 *      takes no stream argument: it enqueues on the handle's own stream and reports through gel_sync(src, NULL). ---- */
int gel_propagate_adjoint(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp /* or NULL */,
                          const double* lam, double* y, double* gx, double* gdisp /* or NULL */);
int gel_propagate_adjoint_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x,
                                 const double* d_disp /* or NULL */, const double* d_lam, double* d_y, double* d_gx,
                                 double* d_gdisp /* or NULL */);
/* info [3]: workspace bytes per lane (vector, functional), lanes per slab a call will use NOW, slabs of a call of B vectors;
 * refuses what the calls refuse, except that it works on GEL_DEVICE_NONE handles */
int gel_prop_adjoint_info(const gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, int64_t* info /* [3] */);

/* ---- one optimiser callback = one device round trip: the four defect groups, the knot / terminal / user row table and the
 *      aero path constraints of ONE decision vector launched back to back on the handle's stream, one synchronise
 *      (what objfunc / sens of Trajectory_Optimization.py:194-312 need from the device).  Every output pointer may be
 *      NULL (= not wanted); vals_full as in gel_eval_jacobian. ---- */
typedef struct {
  double* res;            /* [11N] */
  double* vals_full;      /* [total_nnz] */
  int32_t fill_constants;
  double* rows_con;       /* [nlin + nfn] */
  double* rows_jfn;       /* [nfn][7] */
  double* aero_con[3];    /* per kind */
  double* aero_jac[3];
} gel_callback_io;
int gel_eval_callback(gel_problem* p, const double* x, const gel_callback_io* io);

/* ---- post-processing table (replaces the per-node loop of output_result.py:121-262): for every
 *      state node of the decision vector x, at its time tx_res [M] (seconds: (tau_x (tf - to) / 2 + (tf + to) / 2) unit_t,
 *      Trajectory_Optimization.py:476-491), the derived quantities of the reference's output table, one device thread per
 *      node: out [M][GEL_OUTPUT_COLUMNS] in the order of gel_output_column.  The columns the reference copies from x (time,
 *      mass, position, velocity, quaternion, interpolated body rates) and its text columns (event, stage) stay with the
 *      caller (gelato_amd/output_result.py).  lat_IIP / lon_IIP are NaN where the FAA algorithm has no solution
 *      (posLLH_IIP_FAA(.., fill_na = False)).  launch_*: pdict["LaunchCondition"]["lat" / "lon"] for the downrange. ---- */
#define GEL_OUTPUT_COLUMNS 34
typedef enum {
  GEL_OUT_THRUST = 0, GEL_OUT_LAT, GEL_OUT_LON, GEL_OUT_LAT_IIP, GEL_OUT_LON_IIP, GEL_OUT_DOWNRANGE, GEL_OUT_ALTITUDE,
  GEL_OUT_ALTITUDE_APOGEE, GEL_OUT_ALTITUDE_PERIGEE, GEL_OUT_INCLINATION, GEL_OUT_ARGUMENT_PERIGEE, GEL_OUT_LON_ASCENDING_NODE,
  GEL_OUT_TRUE_ANOMALY, GEL_OUT_VEL_GROUND_NED_X, GEL_OUT_VEL_GROUND_NED_Y, GEL_OUT_VEL_GROUND_NED_Z, GEL_OUT_ACCEL_BODY_X,
  GEL_OUT_AERO_BODY_X, GEL_OUT_HEADING_NED2BODY, GEL_OUT_PITCH_NED2BODY, GEL_OUT_ROLL_NED2BODY,
  GEL_OUT_FLIGHTPATH_VEL_INERTIAL_GEOCENTRIC, GEL_OUT_AZIMUTH_VEL_INERTIAL_GEOCENTRIC, GEL_OUT_THRUST_DIRECTION_ECI_X,
  GEL_OUT_THRUST_DIRECTION_ECI_Y, GEL_OUT_THRUST_DIRECTION_ECI_Z, GEL_OUT_VEL_GROUND, GEL_OUT_VEL_AIR, GEL_OUT_AOA_TOTAL,
  GEL_OUT_AOA_PITCH, GEL_OUT_AOA_YAW, GEL_OUT_DYNAMIC_PRESSURE, GEL_OUT_Q_ALPHA, GEL_OUT_MACH
} gel_output_column;
int gel_output_table(gel_problem* p, const double* x, const double* tx_res /* [M] */, double launch_lat_deg,
                     double launch_lon_deg, double* out /* [M][GEL_OUTPUT_COLUMNS] */);

/* ---- the post-processing table of a BATCH with its Monte-Carlo envelope and the peaks of every flight: what
 *      a dispersed batch of gel_propagate_dispersed* (x_flown = [y | u | t]) is looked at with.
 *      Table: out [B][M][ncols]; out[b][i][c] is what gel_output_table writes for vector b, node i, column cols[c] -- bit for bit,
 *      NaN pattern included -- when disp is NULL and the same tx is given.  cols: ncols distinct gel_output_column values in any
 *      order, or NULL = all 34 in order (ncols is then ignored).  With a subset the kernel leaves out the work only unselected
 *      columns need (Vincenty's iteration, the impact point, the orbital elements); a column that is formed keeps its bits.
 *      Times: tx [B][M] seconds, or NULL: every vector's node times from its own knots and the handle's tau,
 *      (tau_x (tf - to) / 2 + (tf + to) / 2) unit_t with tau_x = [-1, tau], operation for operation the expression of
 *      gelato_amd.output_result.node_times -- the same bits as passing them.
 *      Dispersions: disp [B][S][GEL_PROP_NDISP] or NULL (= all ones), the factors of gel_propagate_dispersed*, each ONE fp64
 *      product formed once per (vector, phase); a factor of exactly 1.0 changes no bit:
 *        index 0  thrust f (column thrust and accel_BODY_X; the nozzle term is untouched)
 *        index 1  mass flow: nothing in the table reads it; IGNORED
 *        index 2  reference_area f (aero_BODY_X, accel_BODY_X)
 *        index 3  wn f, we f on the interpolated wind, before any rotation (dynamic pressure, Q_alpha, the angles of attack, vel_air, M)
 *      Envelope: env [M][ncols][GEL_ENV_NSTAT] = per (node, column), over the vectors b whose entry is finite: count (a double),
 *      mean, m2 = sum (v - mean)^2, min, max, argmin, argmax (vector indices as doubles; compared with < / >: the FIRST vector that
 *      attains the extremum), first_nonfinite (the lowest b whose entry is NaN / Inf, or -1).  count == 0: mean, m2, min, max are
 *      NaN and both arg fields -1; count == 1: m2 is exactly 0.  THE ORDER, a function of the vector index alone: the batch is cut
 *      into blocks of 256 consecutive vectors (block k = vectors 256 k .. 256 k + 255).  Inside a block, Welford's update in
 *      ascending b over the finite entries:  n += 1;  d = v - mean;  mean = mean + d / n;  m2 = fma(d, v - mean, m2).
 *      The blocks that hold a finite entry are merged in ascending k into a running total (the first one is copied), Chan's form:
 *        nt = n + nb;  d = mean_b - mean;  mean = mean + d (nb / nt);  m2 = (m2 + m2_b) + (d d) ((n nb) / nt);  n = nt
 *      each written operation one rounding.  The result does not depend on the stream, the launch geometry or the form (host /
 *      device) of the call, nor on whether out or peaks are asked for too.  No floating-point atomics.  Angle columns are reduced
 *      as the numbers they are: a wrap at +-180 / 360 degrees inside a column's spread is the caller's business.
 *      Peaks: peaks [B][ncols][GEL_PEAK_NSTAT] = per (vector, column), over the nodes in ascending order, finite entries only:
 *      min, its node, max, its node (nodes as doubles; the first node that attains the extremum); NaN and -1 where no node is finite.
 *      A vector's table and peaks depend neither on B nor on its place in the batch.
 *      Status: the table legitimately holds NaN (no impact point), so these calls never return GEL_NONFINITE: count and
 *      first_nonfinite carry that.  GEL_ERR_ARG, decided before the device is looked at: p NULL; B < 0; x NULL with B > 0; cols
 *      given and ncols outside 1 .. 34, a column id out of range or repeated; out, env and peaks all NULL.  On a device handle
 *      also: tables so long that the row tile (64 x 34 doubles) does not fit the workgroup's 64 KB beside them.  A valid call on a
 *      GEL_DEVICE_NONE handle returns what gel_output_table returns there.  B = 0 succeeds and writes the count == 0 envelope when
 *      env is given.  The host form copies in, launches, copies out and synchronises once (the handle's arena).  The device form
 *      takes NO stream argument (a caller-stream form is a later change): like gel_propagate_device it enqueues everything on the
 *      handle's own stream, which is a blocking stream and so orders itself against the null stream, and reports through
 *      gel_sync(p, NULL); a caller on a NON-BLOCKING stream must have finished writing its inputs before the call and must
 *      gel_sync(p, NULL) before it reads the outputs.  cols stays a host pointer in both forms.  The envelope's partials
 *      ([blocks][M][ncols][8] doubles) are the handle's. ---- */
#define GEL_ENV_NSTAT 8  /* count, mean, m2, min, max, argmin, argmax, first_nonfinite */
#define GEL_PEAK_NSTAT 4 /* min, node of min, max, node of max */
int gel_output_table_batch(gel_problem* p, int32_t B, const double* x /* [B][num_vars] */, const double* tx /* [B][M] or NULL */,
                           const double* disp /* [B][S][GEL_PROP_NDISP] or NULL */, double launch_lat_deg, double launch_lon_deg,
                           int32_t ncols, const int32_t* cols /* [ncols] or NULL = all 34 */, double* out /* [B][M][ncols] or NULL */,
                           double* env /* [M][ncols][GEL_ENV_NSTAT] or NULL */, double* peaks /* [B][ncols][GEL_PEAK_NSTAT] or NULL */);
int gel_output_table_batch_device(gel_problem* p, int32_t B, const double* d_x, const double* d_tx /* or NULL */,
                                  const double* d_disp /* or NULL */, double launch_lat_deg, double launch_lon_deg, int32_t ncols,
                                  const int32_t* cols /* host pointer, or NULL */, double* d_out /* or NULL */,
                                  double* d_env /* or NULL */, double* d_peaks /* or NULL */);

/* ---- a Monte-Carlo batch against an ENSEMBLE of wind profiles: a month of soundings, a synthetic ensemble, the
 *      members of a forecast, one per flight, where gel_propagate_dispersed* can only scale the handle's single profile.
 *      Ensemble: tables [E][Kw][3], E >= 1 members of Kw >= 2 rows each, columns (altitude, wind north, wind east) as in
 *      gel_problem_desc.wind_table; every member has its own altitudes, which must increase strictly (the rule of wind_table; the
 *      first offending member is named in gel_last_error).  Each member is staged as a handle's own table is: its rows followed by
 *      its 2 (Kw - 1) slopes (y[k+1] - y[k]) / (x[k+1] - x[k]), 5 Kw - 2 doubles -- bit for bit the wind part of the tables of a
 *      handle created with that member as wind_table (gel_wind_ensemble_member returns it).  The members live in DEVICE memory, not
 *      in a workgroup's LDS: the table limits of a handle (gel_table_limits) do not apply; E (5 Kw - 2) <= 2^27 doubles and
 *      Kw <= 2^20, beyond which creation returns GEL_ERR_ARG.
 *      Assignment: member [B] (host pointer), one entry per vector of the batch: 0 .. E - 1 selects a member, -1 the handle's own
 *      wind table.  gel_wind_ensemble_assign validates it on the host (GEL_ERR_ARG names the first offending vector; nothing is
 *      enqueued), waits for the calls in flight on the source handle and uploads it to a buffer the ensemble owns: the flight and the
 *      table of a batch read the same assignment, and no kernel forms an address from an unchecked index.
 *      Flight b under member e: every wind lookup of that vector runs through the handle's own expression with the member's rows,
 *      slopes and Kw; atmosphere, CA table, the phase's air switch and everything else stay the handle's, and the dispersion factor
 *      of the wind still multiplies the interpolated components afterwards.  THE CONTRACT, for y, err, out, peaks and env, without a
 *      tolerance: a vector with member[b] = e gets bit for bit what the call without an ensemble returns for the same x and disp row
 *      on a handle created from the same problem with wind_table = tables[e]; a vector with member[b] = -1 gets that call's bits on
 *      this handle; and a vector's result depends neither on B, nor on its place in the batch, nor on the slab size, nor on what its
 *      neighbours are assigned.  Valid in all three propagation modes, with or without disp.
 *      Calls: ens == NULL is exactly gel_propagate_dispersed* / gel_output_table_batch*.  With ens, its assignment must hold exactly
 *      B vectors and it must have been created on the plan's / the call's handle, else GEL_ERR_ARG (decided before the device is
 *      looked at).  B = 0 is valid.  Create, info, member and assign work on a GEL_DEVICE_NONE handle (assign validates and keeps the
 *      count); the four evaluation calls refuse such a handle as gel_propagate* does.  The device forms take NO stream argument:
 *      they enqueue on the handle's own stream and report through gel_sync(p, NULL), like gel_propagate_device and
 *      gel_output_table_batch_device.  Status as in those calls: a non-finite wind entry of a member makes its own flights
 *      non-finite and raises GEL_NONFINITE for the flight; the table calls never return it.  An ensemble is destroyed BEFORE its
 *      source handle. ---- */
typedef struct gel_wind_ensemble gel_wind_ensemble; /* opaque */
int gel_wind_ensemble_create(gel_problem* src, int32_t E, int32_t Kw, const double* tables /* [E][Kw][3] */, gel_wind_ensemble** out);
int gel_wind_ensemble_destroy(gel_wind_ensemble* ens);
/* info [5]: E, Kw, doubles per member (5 Kw - 2), device bytes the ensemble holds, vectors of the current assignment or -1 */
int gel_wind_ensemble_info(const gel_wind_ensemble* ens, int64_t* info /* [5] */);
/* member e as staged: rows [Kw][3] | slopes [Kw - 1][2]; works on GEL_DEVICE_NONE handles */
int gel_wind_ensemble_member(const gel_wind_ensemble* ens, int32_t e, double* staged /* [5 Kw - 2] */);
int gel_wind_ensemble_assign(gel_wind_ensemble* ens, int32_t B, const int32_t* member /* host [B] */);
int gel_propagate_ensemble(gel_prop_plan* plan, int32_t B, const double* x, const double* disp /* or NULL */, gel_wind_ensemble* ens /* or NULL */,
                           double* y, double* err /* or NULL */);
int gel_propagate_ensemble_device(gel_prop_plan* plan, int32_t B, const double* d_x, const double* d_disp /* or NULL */,
                                  gel_wind_ensemble* ens /* or NULL */, double* d_y, double* d_err /* or NULL */);
int gel_output_table_batch_ensemble(gel_problem* p, int32_t B, const double* x, const double* tx /* or NULL */, const double* disp /* or NULL */,
                                    gel_wind_ensemble* ens /* or NULL */, double launch_lat_deg, double launch_lon_deg, int32_t ncols,
                                    const int32_t* cols /* or NULL */, double* out, double* env, double* peaks);
int gel_output_table_batch_ensemble_device(gel_problem* p, int32_t B, const double* d_x, const double* d_tx /* or NULL */,
                                           const double* d_disp /* or NULL */, gel_wind_ensemble* ens /* or NULL */, double launch_lat_deg,
                                           double launch_lon_deg, int32_t ncols, const int32_t* cols /* host pointer, or NULL */,
                                           double* d_out /* or NULL */, double* d_env /* or NULL */, double* d_peaks /* or NULL */);

/* ---- the tangent and the adjoint flight under a wind ensemble: gel_propagate_tangent* and gel_propagate_adjoint*
 *      with every flight's derivative taken under the wind table its vector is assigned.  Every wind lookup of vector b runs through
 *      the member's rows, slopes and Kw in all three places: the value right-hand side, its tangent (the slope of the interval the
 *      value lookup took, zero in the clamped ends) and the adjoint's recomputation of F1 .. F3; atmosphere, CA table and everything
 *      else stay the handle's.  The adjoint's value flight is gel_propagate_ensemble*'s: its checkpoints are that flight's bits.
 *      THE CONTRACT, for y, dy, gx and gdisp, without a tolerance (the contract above, extended): a vector with member[b] = e gets bit
 *      for bit what gel_propagate_tangent* / gel_propagate_adjoint* return for the same x, disp row and seeds / lam on a handle
 *      created from the same problem with wind_table = tables[e]; a vector with member[b] = -1 gets that call's bits on this handle;
 *      y is also gel_propagate_ensemble*'s y.  A (vector, direction) or (vector, functional) slice depends neither on B, P or Q, nor
 *      on its place in the batch, nor on the slab size, nor on shared, nor on what its neighbours are assigned.  The parents'
 *      linearity carries over: a zero seed or lam gives zeros, a seed or lam times 2^k gives the outputs times 2^k bit for bit.
 *      Calls: ens == NULL is exactly gel_propagate_tangent* / gel_propagate_adjoint* (those ARE these calls with NULL).  Refusals
 *      (GEL_ERR_ARG, the reason in gel_last_error, all decided before a buffer or the device is looked at): the parent call's, and
 *      an ensemble created on another handle than the plan's or whose assignment does not hold exactly B vectors; a host-only
 *      handle; the adjoint still refuses GEL_PROP_RESTART_NODE plans.  B = 0 succeeds and touches nothing.  gel_prop_tangent_info /
 *      gel_prop_adjoint_info hold unchanged: the ensemble adds no per-lane workspace.  No stream argument: the calls enqueue on the
 *      handle's own stream and report through gel_sync(src, NULL), like their parents.
 *      Status: a non-finite wind entry of a member makes its own flights' y, dy, gx and gdisp non-finite and raises GEL_NONFINITE;
 *      the other vectors' slices stay valid. ---- */
int gel_propagate_tangent_ensemble(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp /* or NULL */,
                                   const double* dx /* or NULL */, const double* ddisp /* or NULL */, gel_wind_ensemble* ens /* or NULL */,
                                   double* y, double* dy);
int gel_propagate_tangent_ensemble_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x,
                                          const double* d_disp /* or NULL */, const double* d_dx /* or NULL */,
                                          const double* d_ddisp /* or NULL */, gel_wind_ensemble* ens /* or NULL */, double* d_y, double* d_dy);
int gel_propagate_adjoint_ensemble(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp /* or NULL */,
                                   const double* lam, gel_wind_ensemble* ens /* or NULL */, double* y, double* gx, double* gdisp /* or NULL */);
int gel_propagate_adjoint_ensemble_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x,
                                          const double* d_disp /* or NULL */, const double* d_lam, gel_wind_ensemble* ens /* or NULL */,
                                          double* d_y, double* d_gx, double* d_gdisp /* or NULL */);

/* ---- wind-profile sensitivities of the flight: the derivative of the flown trajectory with respect to the VALUES
 *      of the wind table its flight reads -- W [Kw][2], north and east per row -- with the table's altitudes x fixed.  The map is
 *      what is coded: the lookup W[i] + (h - x[i]) slope[i] on the piece i with x[i] < h <= x[i + 1], slope staged as
 *      (W[i + 1] - W[i]) / (x[i + 1] - x[i]), row 0 for h <= x[0] and row Kw - 1 for h > x[Kw - 1], the result times the wind factor
 *      fw.  It is linear in W, so along a seed dW the tangent is that lookup applied to the seed on the piece the value took:
 *        th = (h - x[i]) / (x[i + 1] - x[i]);   fma(th, dW[i + 1] - dW[i], dW[i]) inside;   the end row's seed in a clamped end;
 *      times fw, added to the tangent of the interpolated wind beside wn dfw (not added where it is zero: a zero seed changes no
 *      bit).  The adjoint is the transpose: every reversed air stage's (fw lwn, fw lwe) goes to rows i and i + 1 with the weights
 *      1 - th and th, in a clamped end wholly to the end row.  An air-less phase contributes nothing.
 *      Rows: Kg = gel_prop_wind_rows = the handle's Kw, under an ensemble max(handle's Kw, ensemble's Kw).  A lane's table has
 *      Kw <= Kg rows (the handle's, or its vector's member's): seed rows at or beyond Kw are not read, gwind rows there are +0.0.
 *      dwind [B][P][Kg][2], shared = 1: [P][Kg][2].  gwind [B][Q][Kg][2]: every element is written by every call; a row no stage
 *      touched is +0.0.  The tangent accepts any non-empty subset of the seeds dx, ddisp, dwind.
 *      dwind == NULL / gwind == NULL IS gel_propagate_tangent_ensemble* / gel_propagate_adjoint_ensemble*: the same kernels, the same
 *      bits.  With gwind wanted, y, gx and gdisp are still those bits; with dwind given and zero, dy is.  A slice's bits depend
 *      neither on B, P / Q, its place in the batch, shared, the form of the call nor the slab size; a seed or lam times 2^k gives the
 *      outputs times 2^k bit for bit; under an ensemble a vector with member e gets the bits of a handle created with
 *      wind_table = tables[e].  Accumulation: each (vector, functional) owns one column of a workspace [Kg][2][lanes], zeroed on the
 *      stream, updated by read-add-write in walk order by that lane alone (no atomics); 16 Kg bytes per lane more workspace
 *      (gel_prop_adjoint_wind_info: info[0 .. 2] as gel_prop_adjoint_info with that counted where want_gwind != 0, info[3] = Kg).
 *      Refusals: the parents', decided before a buffer or the device is looked at, with the call's name in gel_last_error.  A
 *      non-finite gwind entry raises GEL_NONFINITE like gx.  No stream argument, as in the parents. ---- */
int gel_prop_wind_rows(const gel_prop_plan* plan, const gel_wind_ensemble* ens /* or NULL */, int32_t* Kg);
int gel_propagate_tangent_wind(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* x, const double* disp /* or NULL */,
                               const double* dx /* or NULL */, const double* ddisp /* or NULL */, const double* dwind /* or NULL */,
                               gel_wind_ensemble* ens /* or NULL */, double* y, double* dy);
int gel_propagate_tangent_wind_device(gel_prop_plan* plan, int32_t B, int32_t P, int32_t shared, const double* d_x,
                                      const double* d_disp /* or NULL */, const double* d_dx /* or NULL */, const double* d_ddisp /* or NULL */,
                                      const double* d_dwind /* or NULL */, gel_wind_ensemble* ens /* or NULL */, double* d_y, double* d_dy);
int gel_propagate_adjoint_wind(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* x, const double* disp /* or NULL */,
                               const double* lam, gel_wind_ensemble* ens /* or NULL */, double* y, double* gx, double* gdisp /* or NULL */,
                               double* gwind /* or NULL */);
int gel_propagate_adjoint_wind_device(gel_prop_plan* plan, int32_t B, int32_t Q, int32_t shared, const double* d_x,
                                      const double* d_disp /* or NULL */, const double* d_lam, gel_wind_ensemble* ens /* or NULL */,
                                      double* d_y, double* d_gx, double* d_gdisp /* or NULL */, double* d_gwind /* or NULL */);
int gel_prop_adjoint_wind_info(const gel_prop_plan* plan, const gel_wind_ensemble* ens /* or NULL */, int32_t B, int32_t Q, int32_t shared,
                               int32_t want_gwind, int64_t* info /* [4] */);

/* ---- exact quantiles over the vectors of a batch: what a Monte-Carlo batch is read by -- the 99.865 % value of
 *      every flight's peak, the 0.135 % / 99.865 % band of the terminal row, the 2.5 .. 97.5 % band of every column along the
 *      trajectory, and which flight that is.  src [B][ld]: columns 0 .. W - 1 of every row are read.  Everything below is per column
 *      w, independent of every other column, of W, of ld and of the order of the vectors.
 *      Key: an entry with bits u (uint64) has the key  u ^ (u >> 63 ? ~0 : 1 << 63).  Ascending keys are ascending doubles, with
 *      -0.0 before +0.0.  This total order is the contract.
 *      Which entries count: the finite ones; NaN and +-Inf are left out, as in the envelope.  n = their number; count[w] = n (a double).
 *      The rank rule, for every probs[j]:  h = probs[j] * (double)(n - 1), one fp64 product, one rounding;  lo = floor(h), hi = ceil(h).
 *      Outputs: q[w][j][0] = the lo-th and q[w][j][1] = the hi-th finite entry in key order (0-based), both bit copies of source
 *      entries; n = 0: NaN in both.  who[w][j][.] = the lowest vector index b whose entry has exactly that key, as a double; -1
 *      where n = 0.  The interpolated quantile lower + (upper - lower) (h - lo) is NOT formed here: that is the caller's (Python's).
 *      Being order statistics, the results depend on no summation order, launch geometry, stream or form of the call: they are the
 *      bits a plain sort of the keys gives.  Nothing is sorted and no transposed copy of the source is kept: the call reads the
 *      source three times (range; histogram of GEL-internal 256 bins per column through a monotone map in value space; gather of
 *      the bins that hold a rank), a fourth time when who is given, and a target whose bin holds more than 2048 entries (heavy
 *      ties, one wild vector stretching the range, a range that overflows) is found by bisection on the key over its column, 256
 *      pivots (one byte of the key) per counting round: at most 8 rounds.  No floating-point atomics.
 *      Views: ld >= W lets a call read a view -- the whole table of gel_output_table_batch (W = ld = M ncols), its last node's row
 *      (src + (M - 1) ncols, W = ncols, ld = M ncols), the peaks (W = ld = 4 ncols), err of gel_propagate*, the rows of
 *      gel_rows_eval_device.  All offsets are 64-bit.
 *      GEL_ERR_ARG, decided before the device is looked at: p NULL; B < 0, W < 0, ld < W; src NULL with B W > 0; q NULL; nq outside
 *      1 .. GEL_QUANT_MAXQ; probs NULL, or a probability that is not finite or lies outside [0, 1].  B = 0 succeeds and writes the
 *      n = 0 pattern; W = 0 succeeds and writes nothing.  The source legitimately holds NaN, so these calls never return
 *      GEL_NONFINITE: count carries that.  A valid call on a GEL_DEVICE_NONE handle returns what gel_output_table_batch returns there.
 *      The host form copies rows [B][ld] (up to the last column read) in, launches, copies out and synchronises once (the handle's
 *      arena).  The device form takes NO stream argument: like gel_output_table_batch_device it enqueues everything on the handle's
 *      own stream and reports through gel_sync(p, NULL); there is no host round trip in it.  probs stays a host pointer in both.
 *      Workspace: the handle's, only grows, at most 256 MiB (gel_quantiles_info.workspace_cap_bytes): per column 1048 bytes and
 *      per (column, rank) 16416 bytes; a source wider than fits is walked in slabs of columns (a multiple of 64) on the stream.
 *      gel_batch_quantiles_info (needs no GPU) reports what a call would select.  gel_batch_quantiles_last waits for the handle's
 *      stream and reports how the (column, rank) pairs of the LAST call were settled: stats[0] = their number (2 nq W), [1] by the
 *      range pass alone (n = 0, or a constant column), [2] from a candidate buffer, [3] by the bisection over the column. ---- */
#define GEL_QUANT_MAXQ 16
typedef struct {
  int64_t bins;                /* bins of a column's histogram */
  int64_t cap;                 /* keys a candidate buffer holds: a fuller bin goes to the bisection over the column */
  int64_t chunk;               /* vectors per workgroup of the passes over the source (1024; 256 below 16 column blocks) */
  int64_t slab_cols;           /* columns per slab: the most the workspace cap holds for this nq, a multiple of 64 */
  int64_t workspace_bytes;     /* what this call needs of the handle's workspace */
  int64_t workspace_cap_bytes; /* the cap */
  int64_t passes;              /* reads of the source without who (who adds one); the bisection's rounds are not counted */
  int64_t slabs;               /* slabs this call walks */
} gel_quantiles_info;
int gel_batch_quantiles(gel_problem* p, int32_t B, int64_t W, int64_t ld, const double* src /* [B][ld], columns 0 .. W-1 read */,
                        int32_t nq, const double* probs /* [nq], host */, double* q /* [W][nq][2] */,
                        double* count /* [W] or NULL */, double* who /* [W][nq][2] or NULL */);
int gel_batch_quantiles_device(gel_problem* p, int32_t B, int64_t W, int64_t ld, const double* d_src, int32_t nq,
                               const double* probs /* host */, double* d_q, double* d_count /* or NULL */, double* d_who /* or NULL */);
int gel_batch_quantiles_info(const gel_problem* p, int32_t B, int64_t W, int32_t nq, gel_quantiles_info* info);
int gel_batch_quantiles_last(gel_problem* p, int64_t* stats /* [4] */);

/* ---- co-moments over the vectors of a batch: how two columns move together -- the covariance matrix of the
 *      insertion state, the correlation of max-Q with the terminal miss, the regression of the outputs on the dispersion factors
 *      the flights were flown with.  C[i][j] = sum over the counted flights r of (a_i[r] - mean a_i) (b_j[r] - mean b_j).
 *      Views: column i of flight r of a is a[r lda + i inca] (b likewise), inc >= 1, ld >= (W - 1) inc + 1, all offsets 64-bit.  One
 *      call reads without a copy: disp (W = ld = 4 S); the last node's row of the batch table (src + (M - 1) ncols, W = ncols,
 *      ld = M ncols); the whole table; every flight's maximum out of peaks [B][ncols][4] (src + 2, inc = 4, W = ncols, ld = 4 ncols);
 *      err's last row; the row table.
 *      Which flights count: LISTWISE.  Flight r counts if and only if every entry the call reads of it, in both views, is finite.
 *      (A matrix assembled from pairwise-complete pairs need not be positive semidefinite; the caller chooses columns that are
 *      finite, as cols of gel_output_table_batch lets them.)  info[0] = the count (a double), info[1] = the lowest r left out, or -1.
 *      With a count of 0, C and stat are NaN; with a count of 1 they are C = 0, m2 = 0.  These calls never return GEL_NONFINITE: a
 *      product that overflows is the result.
 *      THE ORDER, a function of the vector index and the set of counted flights alone.  Blocks k = vectors 256 k .. 256 k + 255.
 *      Inside a block, over the counted flights in ascending r, with n, every m, s and C starting at 0:
 *        n += 1
 *        every a column i:  da_i = a_i - ma_i;  ma_i = ma_i + da_i / n;  ea_i = a_i - ma_i;  sa_i = fma(da_i, ea_i, sa_i)
 *        every b column j:  db_j = b_j - mb_j;  mb_j = mb_j + db_j / n;  eb_j = b_j - mb_j;  sb_j = fma(db_j, eb_j, sb_j)
 *        every pair:        C_ij = fma(da_i, eb_j, C_ij)
 *      The blocks that hold a counted flight are merged in ascending k into a running total (the first such block is copied);
 *      every d is formed from the means BEFORE this merge's own mean update:
 *        nt = n + nb;  da_i = ma_b,i - ma_i;  db_j = mb_b,j - mb_j;  w = (n nb) / nt
 *        C_ij = (C_ij + Cb_ij) + (da_i db_j) w
 *        sa_i = (sa_i + sab_i) + (da_i da_i) w          (sb likewise)
 *        ma_i = ma_i + da_i (nb / nt)                   (mb likewise);   n = nt
 *      each written operation one rounding.  stat_a[i] = {ma_i, sa_i}, stat_b[j] = {mb_j, sb_j}: the envelope's mean and m2 of that
 *      column, bit for bit, whenever the counted flights are exactly the column's finite ones.
 *      Self form (b == NULL; Wb, incb, ldb ignored): b is a.  Only the pairs i <= j are formed, C[j][i] is a bit copy of C[i][j], so
 *      C [Wa][Wa] is symmetric in bits, and its diagonal is sa_i by construction.  stat_b must be NULL.
 *      The result does not depend on the stream, the launch geometry, the tile sizes, the slab walk, the workspace size or the form
 *      (host / device) of the call, nor on Wa and Wb beyond the listwise rule: a pair's value depends only on its two columns and
 *      on the set of counted flights.  No floating-point atomics.
 *      GEL_ERR_ARG, decided before the device is looked at: p NULL; B < 0; W < 0; inc < 1; ld < (W - 1) inc + 1 (W > 0); a NULL with
 *      B Wa > 0; C NULL with Wa Wb > 0; info NULL; stat_b given in the self form.  B = 0 succeeds and writes the count = 0 pattern;
 *      Wa = 0 or Wb = 0 succeeds and writes info only.  A valid call on a GEL_DEVICE_NONE handle returns what gel_output_table_batch
 *      returns there.  The host form copies the rows of both views in as they lie (up to the last entry read), launches, copies out
 *      and synchronises once (the handle's arena).  The device form takes NO stream argument: like gel_batch_quantiles_device it
 *      enqueues everything on the handle's own stream and reports through gel_sync(p, NULL).
 *      Workspace: the handle's, only grows, at most 256 MiB (gel_comoments_info.workspace_cap_bytes): one byte per vector, per block
 *      of 256 vectors 16 bytes per column and 8 bytes per pair of the slab.  A product wider than that holds is walked in slabs of
 *      b columns (and, where all a columns beside one tile of b still do not fit, of a columns) on the stream; a call whose fixed
 *      part leaves no room for one tile of pairs is refused (GEL_ERR_ARG).  gel_batch_comoments_info (needs no GPU) reports what a
 *      call would select. ---- */
typedef struct {
  int64_t block;               /* vectors per block of the stated order (256) */
  int64_t tile_a, tile_b;      /* columns of a and of b per workgroup */
  int64_t slab_rows;           /* a columns per slab (Wa unless the cap binds) */
  int64_t slab_cols;           /* b columns per slab */
  int64_t slabs;               /* slabs this call walks */
  int64_t workspace_bytes;     /* what this call needs of the handle's workspace */
  int64_t workspace_cap_bytes; /* the cap */
  int64_t passes_a, passes_b;  /* reads of an entry of a / of b: the mask pass and one per tile of the other view's columns */
} gel_comoments_info;
int gel_batch_comoments(gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const double* a, int64_t Wb, int64_t incb,
                        int64_t ldb, const double* b /* or NULL = the self form */, double* C /* [Wa][Wb]; self form [Wa][Wa] */,
                        double* stat_a /* [Wa][2] mean, m2, or NULL */, double* stat_b /* [Wb][2] or NULL */,
                        double* info /* [2] count, first_excluded */);
int gel_batch_comoments_device(gel_problem* p, int32_t B, int64_t Wa, int64_t inca, int64_t lda, const double* d_a, int64_t Wb,
                               int64_t incb, int64_t ldb, const double* d_b, double* d_C, double* d_stat_a, double* d_stat_b,
                               double* d_info);
int gel_batch_comoments_info(const gel_problem* p, int32_t B, int64_t Wa, int64_t Wb, int32_t self, gel_comoments_info* out);

/* ---- from-file initial guess on the host (replaces initialize.py:322-409 initialize_xdict_6DoF_from_file, LGR mode;
 *      SURVEY.md 8f row f-3): linear interpolation (scipy interp1d with fill_value="extrapolate": the end intervals extend
 *      beyond the table) of a reference trajectory at the state-node times [-1, tau] and the control-node times tau of
 *      every phase, normalised by the handle's units.  table [nref][13] = mass | pos_ECI xyz | vel_ECI xyz | quat_ECI2BODY
 *      wxyz | rate_BODY_Y, rate_BODY_Z.  x = the packed decision vector.  Host arithmetic; works on host-only handles. ---- */
int gel_initial_guess(const gel_problem* p, int32_t nref, const double* t_ref, const double* table /* [nref][13] */,
                      const double* knot_times /* [S+1], seconds */, double* x /* [num_vars] */);

/* ---- node-batched RHS, host buffers (replace dynamics_c.dynamics_velocity,
 *      dynamics_velocity_NoAir, dynamics_quaternion; src/pybind_dynamics.cpp:30,73,94) ---- */
int gel_dynamics_velocity(int32_t n, const double* mass_e, const double* pos_eci_e, const double* vel_eci_e,
                          const double* quat_eci2body, const double* t, const double* param /* [5] */,
                          const double* wind_table, int32_t wind_rows, const double* ca_table, int32_t ca_rows,
                          const double* units /* [3] */, double barC20, double* acc_out /* [n][3] */);
int gel_dynamics_velocity_NoAir(int32_t n, const double* mass_e, const double* pos_eci_e,
                                const double* quat_eci2body, const double* param, const double* units,
                                double barC20, double* acc_out);
int gel_dynamics_quaternion(int32_t n, const double* quat_eci2body, const double* u_e, double unit_u,
                            double* dquat_out /* [n][4] */);

/* ---- device point functions (parity hooks for SURVEY.md 8a rows a4..a9).
 *  kind 0: geometric alt -> [geopotential alt, T, P, rho, a]   in [n]      out [n][5]  (src/Air.cpp:47-111)
 *  kind 1: ECEF xyz      -> [lat deg, lon deg, alt m]          in [n][3]   out [n][3]  (wrapper_coordinate.hpp:105-111)
 *  kind 2: pos           -> gravity                            in [n][3]   out [n][3]  (src/gravity.cpp:11-57), aux[0]=barC20
 *  kind 3: (pos,t,wn,we) -> quatrot(quat_nedg2eci(pos,t),(wn,we,0)) in [n][6] out [n][3] (src/Coordinate.cpp:104-110,
 *                                                                                    src/pybind_dynamics.cpp:51-52)
 *  kind 4: (vel,pos,t)   -> vel_eci2ecef                       in [n][7]   out [n][3]  (src/Coordinate.cpp:69-73)
 *  kind 5: altitude      -> wind_ned, table in aux [K][3]      in [n]      out [n][3]  (wrapper_utils.hpp:82-87)
 *  kind 6: x             -> interp(x, aux[:,0], aux[:,1])      in [n]      out [n]     (wrapper_utils.hpp:51-80)
 *  kind 7: (a, b)        -> [fsqrt(a), sqrt(a), fdiv(a,b), a/b]  in [n][2]   out [n][4]  self-check of the path's guard-free
 *                           fp64 sqrt/division (csrc/gel_physics.h) against the compiler's sequences
 *  kind 8: (angle, ratio) -> [fsin, fcos, sin, cos, flog, log]       in [n][2]   out [n][6]  the path's sincos / log
 *                           (csrc/gel_physics.h: fsincos, flog_ratio) beside the library's
 *  kind 9: 8 abscissae     -> kind 6 of each, looked up one after the other through the table interval kept from the
 *                           previous lookup (what the fused kernel does across a node's sweeps)   in [n][8]  out [n][8]
 *  kind 10: 8 altitudes    -> kind 5 (wn, we) of each, likewise                                    in [n][8]  out [n][16]
 *  kind 11: (q, p)       -> quatmult(q, p)                      in [n][8]   out [n][4]  (src/wrapper_coordinate.hpp:50-57)
 *  kind 12: (q, v)       -> quatrot(q, v) = vec(conj(q) (0, v) q)  in [n][7]  out [n][3]  (:70-78)
 *  kind 13: q            -> [conj(q), thrust direction quatrot(conj(q), (1, 0, 0))]  in [n][4]  out [n][7]  (:59-61,
 *           src/pybind_dynamics.cpp:62-63)
 *  kind 14: x            -> [fexp(x), exp(x)]                    in [n][1]   out [n][2]  self-check of the path's exp
 *  kind 15: (r, kk, dlt)  -> one position sweep in exact-difference form as the fused kernel chains it (csrc/gel_rhs_parts.h:
 *           pos_part of the centre r [m], pos_centre_tail, pos_delta for component kk = 0, 1, 2 moved by dlt [m]), wind table in
 *           aux [K][3]: [rho, P, 1/a, wn, we, sin(lat/2), cos(lat/2), 1/p] of the centre, the same eight of the perturbed point,
 *           pos_delta's return value (1.0: the difference form holds, 0.0: the caller recomputes), the centre's margin [m]
 *                                                                   in [n][5]   out [n][18]
 *           (the half-latitude pair is formed for this hook alone: the position part carries sin / cos of the latitude itself)
 *  kind 16: (r, -, dlt)   -> kind 15's 18 outputs for kk = 0, 1, 2 from ONE centre, as the fused kernel chains its three position
 *           sweeps: 1/T and the margin taken once (pos_centre_tail) and kept, every sweep re-deriving only the wind slopes and the
 *           centre's wind (pos_centre_tail_kept); bit for bit kind 15's             in [n][5]   out [n][3][18]
 */
int gel_point_eval(int32_t kind, int32_t n, const double* in, const double* aux, int32_t aux_rows, double* out);

/* ---- limits of the wind and CA tables.  Every kernel that evaluates aerodynamics keeps the tables in a workgroup's LDS:
 *  T = 85 + 5 wind_rows + 3 ca_rows doubles (atmosphere 88 | wind rows | CA rows | their slopes), beside the launch's own LDS.
 *  No launch asks for more than the 64 KB a workgroup gets without launch attributes; a call whose launch would need more
 *  returns GEL_ERR_ARG before anything is enqueued, and gel_last_error() states the table doubles asked for and those that fit:
 *  gel_problem_create for the fused kernel (T <= 3328) and the aero / callback kernels (T <= 1792, e.g. 320 wind and 32 CA
 *  rows), which also covers the launches that keep nothing behind the tables (exact Jacobians, propagation, output table:
 *  T <= 8192); gel_mesh_error[_device] for the estimate, whose workgroup takes as many vectors of a phase as fit beside the
 *  tables and needs room for one (T <= 8170 - 13 n, below the aero limit only from n = 491 on; the handle stays usable for
 *  everything else); gel_dynamics_velocity (T <= 8192) and gel_point_eval kinds 5, 6, 9, 10, 15, 16 (88 + 5 aux_rows <= 8192) for theirs.
 *  gel_table_limits (needs no GPU): info[0] = T, info[1] = the T that fits the fused kernel, [2] the aero and callback kernels,
 *  [3] one vector of the collocation error estimate of a phase of n nodes (-1 if n is outside 2 .. 511), [4] the launches with nothing
 *  behind the tables, [5] = the cap in bytes, [6] the vectors a workgroup of the estimate takes of such a phase beside these tables
 *  (512 / (n + 1), or fewer where the LDS binds; -1 like [3]). */
int gel_table_limits(int32_t wind_rows, int32_t ca_rows, int32_t n, int64_t* info /* [7] */);

const char* gel_last_error(void);
const char* gel_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GELATO_AMD_H_ */
