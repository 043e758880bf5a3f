// gel_kernels_coo.hip -- the full COO value buffers: compact Jacobian values + constant template -> full values (expand_kernel), the
// constant template alone (fill_full_kernel), the x-dependent entries into a buffer that holds the constants (update_full_kernel,
// update_lines_kernel), and the unpacking of the unit-sharded exchange buffer (shard_unpack_kernel), with their launchers.
#include "gel_tables.h"

namespace gel {

// ---------------------------------------------------------------------------
// compact -> full COO values.  src[i] = -1: constant cval[i]; s >= 0: jvar[b][s]; s <= -2: -jvar[b][-2 - s].
// Two doubles (16 B) per lane: wide coalesced stores.  A thread keeps its two template entries
// (cval, src: 12 B per entry, 7.3 MB at 6x64 -- larger than one XCD's L2) in registers and re-uses them
// for kExpandGroup decision vectors, so the template is read once per group instead of once per vector
// and the kernel is bounded by its 8 B/entry of HBM writes (5.8 TB/s with non-temporal stores).
// ---------------------------------------------------------------------------
constexpr int kExpandGroup = 8;
__global__ __launch_bounds__(kBlock) void expand_kernel(long long nnz, long long V, int B, const double* __restrict__ cval,
                                                        const int32_t* __restrict__ src,
                                                        const double* __restrict__ jvar, double* __restrict__ full) {
  const int b0 = blockIdx.y * kExpandGroup;
  const int nb = min(kExpandGroup, B - b0);
  const bool even = (nnz & 1) == 0;  // then every vector's slice starts 16-byte aligned
  for (long long i = 2 * ((long long)blockIdx.x * kBlock + threadIdx.x); i < nnz; i += 2LL * gridDim.x * kBlock) {
    const bool two = i + 1 < nnz;
    const int s0 = src[i], s1 = two ? src[i + 1] : -1;
    const double c0 = (s0 == -1) ? cval[i] : 0.0, c1 = (two && s1 == -1) ? cval[i + 1] : 0.0;
    const int g0 = (s0 >= 0) ? s0 : -2 - s0, g1 = (s1 >= 0) ? s1 : -2 - s1;  // compact index (unused for constants)
    for (int g = 0; g < nb; g++) {
      const double* jv = jvar + (size_t)(b0 + g) * V;
      double* out = full + (size_t)(b0 + g) * nnz + i;
      const double v0 = (s0 == -1) ? c0 : ((s0 >= 0) ? jv[g0] : -jv[g0]);
      const double v1 = (s1 == -1) ? c1 : ((s1 >= 0) ? jv[g1] : -jv[g1]);
      if (two && (even || ((b0 + g) & 1) == 0)) {
        // written once, read by someone else later: non-temporal (4.2 -> 5.8 TB/s measured)
        typedef double gel_d2 __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(gel_d2{v0, v1}, reinterpret_cast<gel_d2*>(out));
      } else {
        __builtin_nontemporal_store(v0, out);
        if (two) __builtin_nontemporal_store(v1, out + 1);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Update of a full COO value buffer that already holds the constants: only the x-dependent
// entries are written -- full[b][vdst[i]] = +-jvar[b][|vsrc[i]|] for the nvar entries the gather map takes from the compact
// vector (26 k of the 607 k at mixed-6x64), vdst ascending, so the runs that are contiguous in the reference's emission order
// (the [node][xyz] blocks: four fifths of the entries) are coalesced stores and the rest (the diagonal of the dense velocity
// blocks, the pairs of the quaternion blocks) are single 8 / 16-byte writes.  4 % of the bytes expand_kernel writes.
// fill_full_kernel lays the constant template down once (or again whenever the buffer is re-used for other data).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void update_full_kernel(long long nnz, long long V, int nvar, int B, const int32_t* __restrict__ vdst,
                                                             const int32_t* __restrict__ vsrc, const double* __restrict__ jvar,
                                                             double* __restrict__ full) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= nvar) return;
  const int d = vdst[i], s = vsrc[i];
  const int g = (s >= 0) ? s : -2 - s;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const double v = jvar[(size_t)b * V + g];
    full[(size_t)b * nnz + d] = (s >= 0) ? v : -v;
  }
}
// The same update by whole 64-byte lines: every line of a vector's value array that holds at least one x-dependent entry is written
// in full, its constants from the template -- eight lanes per line.  An entry that sits alone between constants (the diagonal of the
// dense velocity blocks: 2,880 per vector at mixed-6x64) is then a full-line write instead of an 8-byte one, which HBM (ECC words of
// 32 / 64 bytes) turns into a read-modify-write: measured 0.26 -> see DESIGN.md ms at B = 1024 for 8 x fewer partial writes.  Needs
// nnz % 8 == 0 (every vector's array starts on a line); launch_update_full() falls back to the entry-wise kernel otherwise.
__global__ __launch_bounds__(kBlock) void update_lines_kernel(long long nnz, long long V, int nlines, int B, const int32_t* __restrict__ vline,
                                                              const int32_t* __restrict__ src, const double* __restrict__ cval,
                                                              const double* __restrict__ jvar, double* __restrict__ full) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 8 * nlines) return;
  const long long i = 8LL * vline[t >> 3] + (t & 7);
  const int s = src[i];
  const double c = (s == -1) ? cval[i] : 0.0;
  const int g = (s >= 0) ? s : -2 - s;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    double v = c;
    if (s != -1) { const double w = jvar[(size_t)b * V + g]; v = (s >= 0) ? w : -w; }
    __builtin_nontemporal_store(v, full + (size_t)b * nnz + i);
  }
}
__global__ __launch_bounds__(kBlock) void fill_full_kernel(long long nnz, int B, const double* __restrict__ cval, double* __restrict__ full) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nnz; i += (long long)gridDim.x * kBlock) {
    const double c = cval[i];
    for (int b = blockIdx.y; b < B; b += gridDim.y) __builtin_nontemporal_store(c, full + (size_t)b * nnz + i);
  }
}

hipError_t launch_expand(long long nnz, long long V, int B, const double* cval, const int32_t* src,
                         const double* d_jvar, double* d_full, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  long long pairs = (nnz + 1) / 2;
  unsigned gx = (unsigned)((pairs + kBlock - 1) / kBlock);
  if (gx > 4096) gx = 4096;
  const int per_launch = 65535 * kExpandGroup;  // grid.y limit
  for (int b0 = 0; b0 < B; b0 += per_launch) {
    const int nb = (B - b0 < per_launch) ? (B - b0) : per_launch;
    hipLaunchKernelGGL(expand_kernel, dim3(gx, (nb + kExpandGroup - 1) / kExpandGroup), dim3(kBlock), 0, s, nnz, V, nb,
                       cval, src, d_jvar + (size_t)b0 * V, d_full + (size_t)b0 * nnz);
  }
  return hipGetLastError();
}

hipError_t launch_update_full(long long nnz, long long V, int nvar, int B, const int32_t* vdst, const int32_t* vsrc,
                              int nlines, const int32_t* vline, const int32_t* src, const double* cval,
                              const double* d_jvar, double* d_full, hipStream_t s) {
  if (B <= 0 || nvar <= 0) return hipSuccess;
  if (nlines > 0 && (nnz & 7) == 0 && ((uintptr_t)d_full & 63) == 0) {
    const unsigned gx = (unsigned)((8LL * nlines + kBlock - 1) / kBlock);
    const unsigned gy = (unsigned)std::min<long long>(B, std::max<long long>(1, 16384 / gx));
    hipLaunchKernelGGL(update_lines_kernel, dim3(gx, gy), dim3(kBlock), 0, s, nnz, V, nlines, B, vline, src, cval, d_jvar, d_full);
    return hipGetLastError();
  }
  const unsigned gx = (unsigned)((nvar + kBlock - 1) / kBlock);
  // enough workgroups to fill the chip whatever the batch; every workgroup strides over the vectors
  const unsigned gy = (unsigned)std::min<long long>(B, std::max<long long>(1, 8192 / gx));
  hipLaunchKernelGGL(update_full_kernel, dim3(gx, gy), dim3(kBlock), 0, s, nnz, V, nvar, B, vdst, vsrc, d_jvar, d_full);
  return hipGetLastError();
}
hipError_t launch_fill_full(long long nnz, int B, const double* cval, double* d_full, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  unsigned gx = (unsigned)((nnz + kBlock - 1) / kBlock);
  if (gx > 2048) gx = 2048;
  hipLaunchKernelGGL(fill_full_kernel, dim3(gx, (unsigned)std::min(B, 16)), dim3(kBlock), 0, s, nnz, B, cval, d_full);
  return hipGetLastError();
}

// pos[i] = rank * width + offset of output entry i (res entries first, then compact Jacobian values): entry i of vector b
// sits at out[(rank * B + b) * width + offset]
__global__ __launch_bounds__(kBlock) void shard_unpack_kernel(long long nres, long long V, long long width, int B,
                                                              const int64_t* __restrict__ pos, const double* __restrict__ out,
                                                              double* __restrict__ res, double* __restrict__ jvar) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nres + V) return;
  if ((i < nres) ? (res == nullptr) : (jvar == nullptr)) return;
  const long long pz = pos[i], r = pz / width, off = pz - r * width;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const double v = out[((size_t)r * B + b) * width + off];
    if (i < nres) res[(size_t)b * nres + i] = v;
    else jvar[(size_t)b * V + (i - nres)] = v;
  }
}

hipError_t launch_shard_unpack(long long nres, long long V, long long width, int B, const int64_t* pos, const double* out,
                               double* d_res, double* d_jvar, hipStream_t s) {
  const unsigned gx = (unsigned)((nres + V + kBlock - 1) / kBlock);
  const unsigned gy = (unsigned)std::min(B, 4096);
  hipLaunchKernelGGL(shard_unpack_kernel, dim3(gx, gy), dim3(kBlock), 0, s, nres, V, width, B, pos, out, d_res, d_jvar);
  return hipGetLastError();
}

}  // namespace gel
