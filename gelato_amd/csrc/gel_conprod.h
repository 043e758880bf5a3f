// gel_conprod.h -- the batched products y = K v and g = K^T lambda with the Jacobian K of every row that is not a defect row
// (the row table's linear and node-function rows, the three aero kinds; gel_kernels_conprod.hip): the tables
// and the launcher.  The tables travel in a struct of their own, as JprodDev does, so that ProblemDev keeps its layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gel {

// Where an entry of K takes its value from (ConprodOpDev::src)
enum : int32_t { kConSrcConst = 0, kConSrcJfn = 1, kConSrcAero0 = 2 /* + kind */ };

// One direction of the operator, compressed by OUTPUT (rows of K for K v, columns for K^T lambda): output o is the fma chain,
// from +0.0, over its entries ptr[o] .. ptr[o + 1] - 1 in table order, out[o] = sum_e value(e) * in[idx[e]], with
//   value(e) = cval[e]                                   src[e] == kConSrcConst  (a linear row's coefficient)
//            = jfn[b][off[e]]                            src[e] == kConSrcJfn    (off = 7 r + c)
//            = aero[kind][b * stride[kind] + off[e]]     src[e] == kConSrcAero0 + kind
// off is the dense table (an element of gel_eval_aero_all_device's jac[kind]) or the record table (an element of the record of
// gel_eval_batch_aero_device); the launcher's caller hands over the one that matches the values it was given.  An entry whose
// record index is -1 (a structural zero) is in neither table, so both name the same entries in the same order.
struct ConprodOpDev {
  int32_t nout, nin;
  const int32_t* ptr;    // [nout + 1]
  const int32_t* idx;    // [nnz] input of the entry
  const int32_t* src;    // [nnz]
  const int64_t* off;    // [nnz] dense or record form
  const double* cval;    // [nnz] the coefficient of a constant entry, 0 elsewhere
};

// The per-vector values of a call: jfn [B][nfn][7]; aero[kind] with stride[kind] doubles per vector (dense: the kind's own array
// and its length; record: the record and its width, three times)
struct ConprodVals {
  const double* jfn;
  int64_t jfn_stride;
  const double* aero[3];
  int64_t aero_stride[3];
};

// out [B][nout] = op applied to in [B][nin]; accumulate != 0: out = fl(out + s), s the value the call writes otherwise.
hipError_t launch_conprod(const ConprodOpDev& op, const ConprodVals& vals, int B, const double* d_in, double* d_out,
                          int accumulate, int32_t* flag, hipStream_t s);

}  // namespace gel
