// gel_kernels_comom.hip -- batched co-moments over the vectors of a batch (gel_batch_comoments*).  fp64, the order of
// include/gelato_amd.h: blocks of 256 consecutive vectors, Welford inside a block over the counted vectors in ascending order, Chan's
// merge of the blocks in ascending order, every written operation one rounding (every product that must not be contracted into the
// sum behind it is a statement of its own: -ffp-contract=on fuses inside one expression only).  No floating-point atomics.
//   comom_mask_kernel    a wavefront per vector: one read of both views, one byte per vector (1 = every entry read of it is finite)
//   comom_count_kernel   one workgroup per block of vectors: the block's count and its lowest excluded vector (integers)
//   comom_info_kernel    count and first_excluded of the call out of the blocks' (integer sums and minima)
//   comom_block_kernel   one workgroup per (block, 32 a columns, 32 b columns): the counted rows of the block, 64 at a time in
//                        ascending order, into LDS; 64 lanes run the per-column chains (one division per step) and leave da and eb
//                        per row in place; every lane then runs the fma chain of its 2 x 2 pairs over the rows
//   comom_merge_kernel   one lane per pair: the blocks' partials in ascending order
//   comom_stats_kernel   one lane per column: mean and m2, the arithmetic of the envelope's merge
#include "gel_comom.h"

namespace gel {
namespace {

__device__ __forceinline__ bool com_finite(double v) {
  return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// true where one of the W entries p[c inc] is NaN or +-Inf: the lanes of a wavefront across the columns, four loads in flight per lane
__device__ __forceinline__ bool com_row_bad(const double* __restrict__ p, long long W, long long inc, int lane) {
  bool bad = false;
  long long c = lane;
  for (; c + 192 < W; c += 256) {
    const double v0 = p[c * inc], v1 = p[(c + 64) * inc], v2 = p[(c + 128) * inc], v3 = p[(c + 192) * inc];
    bad |= !(com_finite(v0) && com_finite(v1) && com_finite(v2) && com_finite(v3));
  }
  for (; c < W; c += 64) bad |= !com_finite(p[c * inc]);
  return bad;
}

// a wavefront per vector (four vectors per workgroup): one read of both views, one byte per vector
__global__ __launch_bounds__(kComThreads) void comom_mask_kernel(ComArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * (kComThreads / 64) + wave;
  if (r >= A.B) return;
  bool bad = false;
  if (A.Wa > 0) bad |= com_row_bad(A.a + r * A.lda, A.Wa, A.inca, lane);
  if (!A.self && A.Wb > 0) bad |= com_row_bad(A.b + r * A.ldb, A.Wb, A.incb, lane);
  const int anybad = __any(bad ? 1 : 0);
  if (lane == 0) A.mask[r] = anybad ? 0 : 1;
}

// one workgroup per block of vectors: the block's count and its lowest excluded vector out of the mask bytes
__global__ __launch_bounds__(kComThreads) void comom_count_kernel(ComArgs A) {
  __shared__ int s_fe;
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * kComBlock;
  const int nr = (int)min((long long)kComBlock, (long long)A.B - r0);
  if (tid == 0) s_fe = INT32_MAX;
  __syncthreads();
  int good = 0;
  if (tid < nr) {
    good = (int)A.mask[r0 + tid];
    if (!good) atomicMin(&s_fe, (int)(r0 + tid));
  }
  const int n = __syncthreads_count(good);
  if (tid == 0) { A.cnt[blockIdx.x] = n; A.fe[blockIdx.x] = s_fe; }
}

__global__ __launch_bounds__(kComThreads) void comom_info_kernel(ComArgs A, int nblk) {
  __shared__ unsigned long long s_n;
  __shared__ int s_fe;
  const int tid = threadIdx.x;
  if (tid == 0) { s_n = 0; s_fe = INT32_MAX; }
  __syncthreads();
  unsigned long long n = 0;
  int fe = INT32_MAX;
  for (int k = tid; k < nblk; k += kComThreads) { n += (unsigned long long)A.cnt[k]; fe = min(fe, A.fe[k]); }
  atomicAdd(&s_n, n);
  atomicMin(&s_fe, fe);
  __syncthreads();
  if (tid == 0) { A.info[0] = (double)s_n; A.info[1] = s_fe == INT32_MAX ? -1.0 : (double)s_fe; }
}

static_assert(kComTileA == 32 && kComTileB == 32 && kComThreads == 256 && kComRows == 64, "the lane maps below are written for these");

__global__ __launch_bounds__(kComThreads) void comom_block_kernel(ComArgs A, long long a0, int an, long long b0, int bn, int nta, int ntb) {
  __shared__ double xa[kComRows * kComTileA];
  __shared__ double xb[kComRows * kComTileB];
  __shared__ int rows[kComBlock];
  __shared__ int wcnt[kComThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntile = nta * ntb;
  const int k = blockIdx.x / ntile, tile = blockIdx.x - k * ntile;
  const int ti = tile / ntb, tj = tile - ti * ntb;
  const long long i0 = a0 + (long long)ti * kComTileA, j0 = b0 + (long long)tj * kComTileB;
  const int wa = (int)min((long long)kComTileA, a0 + an - i0), wb = (int)min((long long)kComTileB, b0 + bn - j0);
  // the self form keeps the pairs i <= j only: a tile wholly below the diagonal has nothing to form, unless it is the one that
  // writes its columns' statistics (the first tile of the slab in either direction)
  if (A.self && ti != 0 && tj != 0 && i0 > j0 + wb - 1) return;
  const long long r0 = (long long)k * kComBlock;
  const int nr = (int)min((long long)kComBlock, (long long)A.B - r0);
  // the counted vectors of the block, in ascending order
  const int good = tid < nr ? (int)A.mask[r0 + tid] : 0;
  const unsigned long long bal = __ballot(good);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int base = 0, n = 0;
#pragma unroll
  for (int w = 0; w < kComThreads / 64; w++) { if (w < wave) base += wcnt[w]; n += wcnt[w]; }
  if (good) rows[base + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
  if (n == 0) return;   // the merge never reads the partials of a block without a counted vector
  __syncthreads();
  // lanes 0 .. 31: the chain of a column 'col'; lanes 32 .. 63: of b column 'col'
  const bool isa = tid < kComTileA;
  const int col = tid & 31;
  const bool chain = tid < 64 && col < (isa ? wa : wb);
  double* const xc = isa ? xa : xb;
  double nn = 0.0, mean = 0.0, m2 = 0.0;
  const int ty = tid >> 4, tx = tid & 15;
  double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
  for (int c0 = 0; c0 < n; c0 += kComRows) {
    const int m = min(kComRows, n - c0);
    for (int e = tid; e < m * kComTileA; e += kComThreads) {
      const int rr = e >> 5, ci = e & 31;
      xa[e] = ci < wa ? A.a[(r0 + rows[c0 + rr]) * A.lda + (i0 + ci) * A.inca] : 0.0;
    }
    for (int e = tid; e < m * kComTileB; e += kComThreads) {
      const int rr = e >> 5, cj = e & 31;
      xb[e] = cj < wb ? A.b[(r0 + rows[c0 + rr]) * A.ldb + (j0 + cj) * A.incb] : 0.0;
    }
    __syncthreads();
    if (chain) {
      for (int rr = 0; rr < m; rr++) {
        // n += 1; d = v - mean; mean = mean + d / n; e = v - mean; m2 = fma(d, e, m2)
        const double v = xc[rr * 32 + col];
        nn += 1.0;
        const double d = v - mean;
        const double q = d / nn;
        mean = mean + q;
        const double e2 = v - mean;
        m2 = __builtin_fma(d, e2, m2);
        xc[rr * 32 + col] = isa ? d : e2;   // da of an a column, eb of a b column
      }
    }
    __syncthreads();
    for (int rr = 0; rr < m; rr++) {   // ascending counted vectors: C_ij = fma(da_i, eb_j, C_ij)
      const double da0 = xa[rr * 32 + 2 * ty], da1 = xa[rr * 32 + 2 * ty + 1];
      const double eb0 = xb[rr * 32 + 2 * tx], eb1 = xb[rr * 32 + 2 * tx + 1];
      c00 = __builtin_fma(da0, eb0, c00);
      c01 = __builtin_fma(da0, eb1, c01);
      c10 = __builtin_fma(da1, eb0, c10);
      c11 = __builtin_fma(da1, eb1, c11);
    }
    __syncthreads();
  }
  double* const cp = A.cp + ((size_t)k * an + (size_t)(i0 - a0)) * (size_t)bn + (size_t)(j0 - b0);
  const int ia = 2 * ty, jb = 2 * tx;
  if (ia < wa && jb < wb) cp[(size_t)ia * bn + jb] = c00;
  if (ia < wa && jb + 1 < wb) cp[(size_t)ia * bn + jb + 1] = c01;
  if (ia + 1 < wa && jb < wb) cp[(size_t)(ia + 1) * bn + jb] = c10;
  if (ia + 1 < wa && jb + 1 < wb) cp[(size_t)(ia + 1) * bn + jb + 1] = c11;
  if (chain && isa && tj == 0) {
    double* const w = A.sa + ((size_t)k * A.Wa + (size_t)(i0 + col)) * 2;
    w[0] = mean; w[1] = m2;
  }
  if (chain && !isa && ti == 0) {
    double* const w = A.sb + ((size_t)k * bn + (size_t)(j0 - b0 + col)) * 2;
    w[0] = mean; w[1] = m2;
  }
}

__global__ __launch_bounds__(kComThreads) void comom_merge_kernel(ComArgs A, long long a0, int an, long long b0, int bn, int nblk) {
  const long long p = (long long)blockIdx.x * kComThreads + threadIdx.x;
  if (p >= (long long)an * bn) return;
  const int ii = (int)(p / bn), jj = (int)(p - (long long)ii * bn);
  const long long i = a0 + ii, j = b0 + jj;
  if (A.self && i > j) return;
  double n = 0.0, ma = 0.0, mb = 0.0, c = 0.0;
  for (int k = 0; k < nblk; k++) {   // ascending block order
    const double nb = (double)A.cnt[k];
    if (nb == 0.0) continue;
    const double mak = A.sa[((size_t)k * A.Wa + (size_t)i) * 2], mbk = A.sb[((size_t)k * bn + jj) * 2];
    const double ck = A.cp[((size_t)k * an + ii) * (size_t)bn + jj];
    if (n == 0.0) { n = nb; ma = mak; mb = mbk; c = ck; continue; }
    // nt = n + nb; da = ma_b - ma; db = mb_b - mb; w = (n nb) / nt; C = (C + C_b) + (da db) w; m = m + d (nb / nt); n = nt
    const double nt = n + nb, da = mak - ma, db = mbk - mb;
    const double fb = nb / nt, w = n * nb / nt;
    const double s = c + ck, pr = da * db;
    const double t = pr * w;
    c = s + t;
    const double dma = da * fb, dmb = db * fb;
    ma = ma + dma;
    mb = mb + dmb;
    n = nt;
  }
  const double r = n == 0.0 ? __builtin_nan("") : c;
  A.C[(size_t)i * A.Wb + (size_t)j] = r;
  if (A.self) A.C[(size_t)j * A.Wb + (size_t)i] = r;   // a bit copy: symmetric in bits
}

// mean and m2 of W columns out of the blocks' statistics part [blocks][W][2] into out [W][2]
__global__ __launch_bounds__(kComThreads) void comom_stats_kernel(const int32_t* __restrict__ cnt, int nblk, long long W,
                                                                  const double* __restrict__ part, double* __restrict__ out) {
  const long long col = (long long)blockIdx.x * kComThreads + threadIdx.x;
  if (col >= W) return;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int k = 0; k < nblk; k++) {
    const double nb = (double)cnt[k];
    if (nb == 0.0) continue;
    const double* const w = part + ((size_t)k * W + (size_t)col) * 2;
    if (n == 0.0) { n = nb; mean = w[0]; m2 = w[1]; continue; }
    const double nt = n + nb, d = w[0] - mean;
    const double fb = nb / nt, fab = n * nb / nt;
    const double dm = d * fb;
    mean = mean + dm;
    const double s2 = m2 + w[1], dd = d * d;
    const double t2 = dd * fab;
    m2 = s2 + t2;
    n = nt;
  }
  const double nan = __builtin_nan("");
  out[col * 2] = n == 0.0 ? nan : mean;
  out[col * 2 + 1] = n == 0.0 ? nan : m2;
}

}  // namespace

hipError_t launch_comom_mask(const ComArgs& A, hipStream_t s) {
  const long long nblk = ((long long)A.B + kComBlock - 1) / kComBlock;
  if (nblk > 0) {
    const long long per = kComThreads / 64;
    hipLaunchKernelGGL(comom_mask_kernel, dim3((unsigned)(((long long)A.B + per - 1) / per)), dim3(kComThreads), 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(comom_count_kernel, dim3((unsigned)nblk), dim3(kComThreads), 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(comom_info_kernel, dim3(1), dim3(kComThreads), 0, s, A, (int)nblk);
  return hipGetLastError();
}

hipError_t launch_comom_slab(const ComArgs& A, int64_t a0, int64_t an, int64_t b0, int64_t bn, hipStream_t s) {
  const long long nblk = ((long long)A.B + kComBlock - 1) / kComBlock;
  const long long nta = (an + kComTileA - 1) / kComTileA, ntb = (bn + kComTileB - 1) / kComTileB;
  const long long grid = nblk * nta * ntb, pairs = (long long)an * bn;
  if (grid > 0x7fffffffLL || nta * ntb > 0x7fffffffLL || an > 0x7fffffffLL || bn > 0x7fffffffLL || (pairs + kComThreads - 1) / kComThreads > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (grid > 0) {
    hipLaunchKernelGGL(comom_block_kernel, dim3((unsigned)grid), dim3(kComThreads), 0, s, A, (long long)a0, (int)an, (long long)b0, (int)bn,
                       (int)nta, (int)ntb);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(comom_merge_kernel, dim3((unsigned)((pairs + kComThreads - 1) / kComThreads)), dim3(kComThreads), 0, s, A, (long long)a0,
                     (int)an, (long long)b0, (int)bn, (int)nblk);
  return hipGetLastError();
}

hipError_t launch_comom_stats(const ComArgs& A, int64_t W, const double* part, double* out, hipStream_t s) {
  if (!out || W <= 0) return hipSuccess;
  const long long nblk = ((long long)A.B + kComBlock - 1) / kComBlock;
  hipLaunchKernelGGL(comom_stats_kernel, dim3((unsigned)((W + kComThreads - 1) / kComThreads)), dim3(kComThreads), 0, s, A.cnt, (int)nblk,
                     (long long)W, part, out);
  return hipGetLastError();
}

}  // namespace gel
