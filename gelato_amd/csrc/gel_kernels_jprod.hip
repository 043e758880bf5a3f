// gel_kernels_jprod.hip -- the batched Jacobian products from the compact values (gel_jac_matvec*, gel_jac_rmatvec*).
//
//   y_b = J(x_b) v_b           y [B][11 N]       g_b = J(x_b)^T lambda_b       g [B][num_vars]
//
// J(x_b) is the matrix the pattern, the constant template and the gather map define when applied to jvar[b]; the full value array
// is never formed.  The tables (gel_jprod.h, built on the host from the pattern walk) hold the non-zero entries only.
//
// One workgroup = (group of VB decision vectors, phase): the products are block-diagonal per phase but for the time columns.  The
// phase's slice of the VB input vectors is staged in LDS as [input][VB]; one lane = one output (row of J v, column of J^T lambda)
// of all VB vectors: every table element (four indices or two coefficients per 16-byte load, coalesced over the wavefront; outputs
// with equal constant coefficients share a coefficient row) feeds VB FMAs from registers, and
// the VB inputs of an entry come with one or a few wide LDS reads (a broadcast where the lanes of a wavefront share the input,
// as along a row of D).  A variable entry reads its compact value once per vector; the lanes of a wavefront walk the nodes of a slot.
// Every output is a sum in a fixed order of its own table row: a vector's results depend neither on its neighbours in the batch nor
// on VB or B.  The time columns of J^T lambda (11 n terms per phase and side) are summed by the whole workgroup: lane t takes the
// terms t, t + lanes, ... in order, then a fixed tree inside each wavefront and the wavefronts in order; the per-phase partials go to a workspace and tsum_kernel adds
// the two phases that share a column, in a fixed order.  No floating-point atomics anywhere.  fp64 throughout.
#include <hip/hip_runtime.h>

#include "gel_jprod.h"

namespace gel {
namespace {

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// The VB staged inputs of one entry, lds[idx * VB ..]: 16-byte reads (ds_read_b128 moves four times the bytes per LDS cycle of the
// ds_read2_b64 the compiler picks for a pointer it only knows to be 8-byte aligned).
typedef double d2_t __attribute__((ext_vector_type(2)));
template <int VB>
__device__ __forceinline__ void load_inputs(const double* lds, int idx, double (&w)[VB]) {
  if constexpr (VB == 1) {
    w[0] = lds[idx];
  } else {
    const d2_t* const p = reinterpret_cast<const d2_t*>(__builtin_assume_aligned(lds + (size_t)idx * VB, 16));
#pragma unroll
    for (int k = 0; k < VB / 2; k++) {
      const d2_t t = p[k];
      w[2 * k] = t.x;
      w[2 * k + 1] = t.y;
    }
  }
}

template <int VB, bool T>
__global__ __launch_bounds__(kJprodMaxThreads) void jprod_kernel(JprodDev Jd, int B, const double* __restrict__ jvar,
                                                              const double* __restrict__ in, double* __restrict__ out,
                                                              double* __restrict__ tpart, int32_t* flag) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int s = blockIdx.x % Jd.S;
  const long long b0 = (long long)(blockIdx.x / Jd.S) * VB;
  const JprodPhaseDev* const ph = Jd.ph + s;
  const JprodOpDev op = T ? ph->bw : ph->fw;
  const int nout = op.nout, nin = op.nin, tid = threadIdx.x, nthreads = blockDim.x;
  const size_t ldin = T ? Jd.nres : Jd.nvars, ldout = T ? Jd.nvars : Jd.nres;
  // the vectors of the group; beyond the batch the last vector is computed again and not stored
  const double* inb[VB];
  const double* jvb[VB];
#pragma unroll
  for (int k = 0; k < VB; k++) {
    const long long b = (b0 + k < B) ? b0 + k : (long long)B - 1;
    inb[k] = in + (size_t)b * ldin;
    jvb[k] = jvar + (size_t)b * Jd.V + ph->voff;
  }
  // ---- stage the phase's inputs: lds[l * VB + k] = in[b0 + k][imap[l]] ----
  const int32_t* const imap = Jd.it + op.imap;
  for (int l = tid; l < nin; l += nthreads) {
    const int g = imap[l];
#pragma unroll
    for (int k = 0; k < VB; k++) lds[(size_t)l * VB + k] = inb[k][g];
  }
  __syncthreads();

  const int32_t* const cnt = Jd.it + op.cnt;
  const int32_t* const cidx = Jd.it + op.cidx;
  const int32_t* const vidx = Jd.it + op.vidx;
  const int32_t* const vslot = Jd.it + op.vslot;
  const int32_t* const omap = Jd.it + op.omap;
  const int32_t* const vrow = Jd.it + op.vrow;
  const double* const cval = Jd.dt + op.cval;
  const int nvr = op.nvr;
  bool bad = false;
  for (int o = tid; o < nout; o += nthreads) {
    double acc[VB];
#pragma unroll
    for (int k = 0; k < VB; k++) acc[k] = 0.0;
    const int nc = cnt[o], nv = cnt[nout + o], vr = vrow[o];
    // four constant entries per step: one 16-byte load of their inputs' indices, two of their coefficients
    int e = 0;
#pragma unroll 2
    for (; e + 4 <= nc; e += 4) {
      const int4 id = *reinterpret_cast<const int4*>(cidx + jprod_cidx_at(e, nout, o));
      const d2_t c01 = *reinterpret_cast<const d2_t*>(cval + jprod_cval_at(e, nvr, vr));
      const d2_t c23 = *reinterpret_cast<const d2_t*>(cval + jprod_cval_at(e + 2, nvr, vr));
      double p0[VB], p1[VB], p2[VB], p3[VB];
      load_inputs<VB>(lds, id.x, p0);
      load_inputs<VB>(lds, id.y, p1);
      load_inputs<VB>(lds, id.z, p2);
      load_inputs<VB>(lds, id.w, p3);
#pragma unroll
      for (int k = 0; k < VB; k++) {
        acc[k] = __builtin_fma(c01.x, p0[k], acc[k]);
        acc[k] = __builtin_fma(c01.y, p1[k], acc[k]);
        acc[k] = __builtin_fma(c23.x, p2[k], acc[k]);
        acc[k] = __builtin_fma(c23.y, p3[k], acc[k]);
      }
    }
    for (; e < nc; e++) {
      const double c = cval[jprod_cval_at(e, nvr, vr)];
      double p[VB];
      load_inputs<VB>(lds, cidx[jprod_cidx_at(e, nout, o)], p);
#pragma unroll
      for (int k = 0; k < VB; k++) acc[k] = __builtin_fma(c, p[k], acc[k]);
    }
    for (e = 0; e < nv; e++) {
      const int sl = vslot[(size_t)e * nout + o];
      double p[VB];
      load_inputs<VB>(lds, vidx[(size_t)e * nout + o], p);
      const int off = sl >> 1;
      const bool neg = sl & 1;
#pragma unroll
      for (int k = 0; k < VB; k++) {
        const double a = jvb[k][off];
        acc[k] = __builtin_fma(neg ? -a : a, p[k], acc[k]);
      }
    }
    const size_t go = (size_t)omap[o];
#pragma unroll
    for (int k = 0; k < VB; k++)
      if (b0 + k < B) {
        out[(size_t)(b0 + k) * ldout + go] = acc[k];
        bad = bad || !finite64(acc[k]);
      }
  }

  if (T) {
    // ---- the two time columns: per-lane strided partial sums, a fixed tree inside each wavefront, then the wavefronts in order ----
    double* const red = lds + (size_t)nin * VB;   // [wavefronts][VB]
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    for (int side = 0; side < 2; side++) {
      const JprodTcolDev tc = ph->tc[side];
      const int32_t* const ridx = Jd.it + tc.ridx;
      const int32_t* const tslot = Jd.it + tc.tslot;
      const double* const tval = Jd.dt + tc.tval;
      double acc[VB];
#pragma unroll
      for (int k = 0; k < VB; k++) acc[k] = 0.0;
      for (int e = tid; e < tc.nt; e += nthreads) {
        const int sl = tslot[e];
        double p[VB];
        load_inputs<VB>(lds, ridx[e], p);
        if (sl < 0) {
          const double c = tval[e];
#pragma unroll
          for (int k = 0; k < VB; k++) acc[k] = __builtin_fma(c, p[k], acc[k]);
        } else {
          const int off = sl >> 1;
          const bool neg = sl & 1;
#pragma unroll
          for (int k = 0; k < VB; k++) {
            const double a = jvb[k][off];
            acc[k] = __builtin_fma(neg ? -a : a, p[k], acc[k]);
          }
        }
      }
#pragma unroll
      for (int st = 32; st > 0; st >>= 1) {
#pragma unroll
        for (int k = 0; k < VB; k++) acc[k] += __shfl_down(acc[k], st, 64);
      }
      __syncthreads();   // (side 1: the partial sums of side 0 have been read)
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < VB; k++) red[wave * VB + k] = acc[k];
      }
      __syncthreads();
      if (tid < VB && b0 + tid < B) {
        double t = red[tid];
        for (int w = 1; w < nwaves; w++) t += red[w * VB + tid];
        tpart[((size_t)(b0 + tid) * Jd.S + s) * 2 + side] = t;
      }
    }
  }
  if (bad) *(volatile int32_t*)flag = 1;
}

// g[b][tcol0 + i] = (tf side of phase i - 1) + (to side of phase i): the two partials of a time column, always in this order
__global__ void tsum_kernel(JprodDev Jd, int B, const double* __restrict__ tpart, double* __restrict__ g, int32_t* flag) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nt = Jd.S + 1;
  if (t >= (long long)B * nt) return;
  const long long b = t / nt;
  const int i = (int)(t - b * nt);
  const double* const pb = tpart + (size_t)b * Jd.S * 2;
  double v;
  if (i == 0) v = pb[0];
  else if (i == Jd.S) v = pb[(size_t)(i - 1) * 2 + 1];
  else v = pb[(size_t)(i - 1) * 2 + 1] + pb[(size_t)i * 2];
  g[(size_t)b * Jd.nvars + Jd.tcol0 + i] = v;
  if (!finite64(v)) *(volatile int32_t*)flag = 1;
}

template <int VB>
hipError_t launch_vb(const JprodDev& Jd, int nin_max, int B, const double* jv, const double* in, double* out, double* tpart,
                     int32_t* flag, int transpose, int threads, hipStream_t s) {
  const long long grid = ((long long)B + VB - 1) / VB * Jd.S;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = jprod_lds_bytes(nin_max, VB, transpose != 0);
  if (lds > kJprodMaxLds) return hipErrorInvalidValue;
  if (transpose) hipLaunchKernelGGL((jprod_kernel<VB, true>), dim3((unsigned)grid), dim3(threads), lds, s, Jd, B, jv, in, out, tpart, flag);
  else hipLaunchKernelGGL((jprod_kernel<VB, false>), dim3((unsigned)grid), dim3(threads), lds, s, Jd, B, jv, in, out, tpart, flag);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_jprod(const JprodDev& Jd, int nin_max, int B, const double* d_jvar, const double* d_in, double* d_out,
                        double* d_tpart, int32_t* flag, int transpose, int vb, int threads, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (threads != 256 && threads != 512) return hipErrorInvalidValue;
  if (vb <= 0) vb = jprod_vectors_per_group(nin_max, transpose != 0);
  hipError_t e;
  switch (vb) {
    case 8: e = launch_vb<8>(Jd, nin_max, B, d_jvar, d_in, d_out, d_tpart, flag, transpose, threads, s); break;
    case 4: e = launch_vb<4>(Jd, nin_max, B, d_jvar, d_in, d_out, d_tpart, flag, transpose, threads, s); break;
    case 2: e = launch_vb<2>(Jd, nin_max, B, d_jvar, d_in, d_out, d_tpart, flag, transpose, threads, s); break;
    case 1: e = launch_vb<1>(Jd, nin_max, B, d_jvar, d_in, d_out, d_tpart, flag, transpose, threads, s); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess || !transpose) return e;
  const long long n = (long long)B * (Jd.S + 1);
  if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Jd, B, d_tpart, d_out, flag);
  return hipGetLastError();
}

}  // namespace gel
