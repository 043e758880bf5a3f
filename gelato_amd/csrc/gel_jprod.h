// gel_jprod.h -- the batched Jacobian products y = J v and g = J^T lambda from the compact values (gel_kernels_jprod.hip;
// DESIGN.md 3.10): their tables and launchers.  The tables travel in a struct of their own (JprodDev), as MeshDev does, so that
// ProblemDev keeps its layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gel {

// One direction of one phase: a sparse operator out[o] = sum_e coef(e) in[idx(e)] over the phase's LOCAL outputs and inputs, stored
// entry-major ("ELL transposed": entry e of output o at [e * nout + o]), so that the lanes of a wavefront -- one output each -- read
// a table row with one coalesced load.  Only non-zero entries are stored; an output's constant entries come first, its variable
// entries (coefficient = +- a compact value) after them, each in the order of the pattern walk.
//   cnt   [2][nout] int32   constant entries, variable entries of every output
//   cidx  [cw4/4][nout][4] int32  local input of a constant entry, four entries of an output side by side (one 16-byte load)
//   cval  [cw4/2][nvr][2] double  its coefficient, two entries side by side, row vrow[o]   (cw4 = cw rounded up to 4; padding 0)
//   vrow  [nout] int32      the output's row of constant coefficients: outputs whose coefficients are the same sequence share one
//                           (the rows of one node's mass, position and quaternion components all carry D[j][0..n]), numbered in
//                           the order of the outputs, so that the lanes of a wavefront read a few neighbouring values
//   vidx  [vw][nout] int32  local input of a variable entry        vslot [vw][nout] int32  2 * (compact slot - voff) + (1 if negated)
//   omap  [nout] int32      global row (J v) or column (J^T lambda) of every local output
//   imap  [nin] int32       global column (J v) or row (J^T lambda) of every local input
struct JprodOpDev {
  int32_t nout, nin, cw, vw, nvr, pad;
  int64_t cnt, cidx, vidx, vslot, omap, imap, vrow;   // offsets (int32 elements) in JprodDev::it
  int64_t cval;                                 // offset (doubles) in JprodDev::dt
};
// The two time columns of a phase (to = column s, tf = column s + 1 of the t block) in J^T lambda: 11 n terms each, summed by the
// whole workgroup in a fixed order (strided partial sums per lane, a fixed tree inside each wavefront, then the wavefronts in order),
// one partial per (vector, phase, side).
//   ridx [nt] int32  local row (input of the transposed operator)    tslot [nt] int32  as vslot, or -1: constant tval [k]
struct JprodTcolDev {
  int32_t nt, pad;
  int64_t ridx, tslot;   // offsets in JprodDev::it
  int64_t tval;          // offset in JprodDev::dt ([nt], 0 where the entry is variable)
};
struct JprodPhaseDev {
  JprodOpDev fw, bw;     // J v (outputs: the phase's 11 n rows; inputs: its columns, the two time columns last); J^T lambda
                         // (outputs: the phase's columns but the time columns; inputs: its rows)
  JprodTcolDev tc[2];
  int64_t voff;          // first compact value of the phase
};

struct JprodDev {
  int32_t S, V, nvars, nres;   // phases, compact values, decision variables, residual rows (11 N)
  int32_t tcol0, pad;          // first global column of the t block
  const JprodPhaseDev* ph;
  const int32_t* it;
  const double* dt;
};

// element of cidx / cval that holds constant entry e of output o / coefficient row vr
inline __host__ __device__ size_t jprod_cidx_at(int e, int nout, int o) { return ((size_t)(e >> 2) * nout + o) * 4 + (e & 3); }
inline __host__ __device__ size_t jprod_cval_at(int e, int nvr, int vr) { return ((size_t)(e >> 1) * nvr + vr) * 2 + (e & 1); }

constexpr int kJprodMaxThreads = 512;        // largest workgroup of jprod_kernel (its launch bound)
constexpr size_t kJprodMaxLds = 64 * 1024;   // LDS a workgroup may take (the default limit of a launch without attributes)

// bytes of LDS a workgroup of vb vectors takes: the staged inputs [nin][vb], and for J^T lambda the wavefronts' partial sums [8][vb]
inline size_t jprod_lds_bytes(int nin_max, int vb, bool transpose) {
  return 8 * ((size_t)nin_max * vb + (transpose ? (size_t)(kJprodMaxThreads / 64) * vb : 0));
}
// vectors per workgroup (8, 4, 2 or 1): the most whose staged inputs fit; 0: none does
inline int jprod_vectors_per_group(int nin_max, bool transpose) {
  for (int vb = 8; vb >= 1; vb >>= 1)
    if (jprod_lds_bytes(nin_max, vb, transpose) <= kJprodMaxLds) return vb;
  return 0;
}

// y [B][nres] = J v (transpose = 0, in = v [B][nvars]) or g [B][nvars] = J^T lambda (transpose = 1, in = lambda [B][nres]);
// tpart [B][S][2]: workspace of the transposed product (the phases' partial sums of the time columns).  nin_max: the largest
// nin of the direction over the phases.  vb: vectors per workgroup (0 = jprod_vectors_per_group); a vector's results do not depend on it.
// threads: 256 or 512 lanes per workgroup (the time columns' summation order follows it: one value per handle, not per call).
hipError_t launch_jprod(const JprodDev& Jd, int nin_max, int B, const double* d_jvar, const double* d_in, double* d_out,
                        double* d_tpart, int32_t* flag, int transpose, int vb, int threads, hipStream_t s);

}  // namespace gel
