// gel_kernels_quant.hip -- exact batched quantiles over the vectors of a batch (gel_batch_quantiles*).
// The k-th smallest finite entry of every column of src [B][ld], by selection: nothing is sorted and no transposed copy is kept.
//   range      n, minimum and maximum key per column                                              (one read of the source)
//   histogram  256 bins per column through a monotone map in value space                          (one read)
//   locate     per (column, rank): the bin that holds it and the rank inside that bin
//   gather     the entries of those bins into a buffer per target                                 (one read)
//   select     the rank inside the buffer, by bisection on the key in the workgroup's LDS
//   fallback   every target whose bin holds more than kQuantCap entries: the key byte by byte, counting over the whole column
//   who        only when asked for: the lowest vector that holds the answer's key                 (one read)
// All decisions are integer comparisons of keys and integer counts; the counts are merged by integer atomics, whose result does
// not depend on the order of arrival.  The bin map is floating point but only has to be monotone: entries of a lower bin have lower
// keys whatever the rounding, so the bin of a rank and the rank inside it are exact.  No floating-point atomics anywhere.
#include "gel_quant.h"

namespace gel {
namespace {

typedef unsigned long long u64;

constexpr u64 kSign = 1ull << 63;
constexpr u64 kExp = 0x7ffull << 52;

__device__ __forceinline__ bool finite_bits(u64 u) { return (u & kExp) != kExp; }
// ascending keys = ascending doubles, -0.0 before +0.0 (the contract of include/gelato_amd.h)
__device__ __forceinline__ u64 key_of(u64 u) { return u ^ ((u >> 63) ? ~0ull : kSign); }
__device__ __forceinline__ u64 bits_of(u64 k) { return k ^ ((k >> 63) ? kSign : ~0ull); }
__device__ __forceinline__ double value_of(u64 k) { return __longlong_as_double((long long)bits_of(k)); }

// The bin map of a column: bin = clamp(floor((v - vmin) scale)), non-decreasing in v under round-to-nearest (a difference with a
// fixed subtrahend, a product with a non-negative factor and the truncation are each non-decreasing).  A range that overflows, or
// one so narrow that the factor would, gives scale = 0: every entry in bin 0, which the candidate buffer or the fallback serves.
struct BinMap { double vmin, scale; };
__device__ __forceinline__ BinMap bin_map(u64 kmin, u64 kmax) {
  BinMap m;
  m.vmin = value_of(kmin);
  const double r = value_of(kmax) - m.vmin;
  const double s = (double)kQuantBins / r;
  const bool ok = r > 0.0 && r <= 1.7976931348623157e308 && s <= 1.7976931348623157e308;
  m.scale = ok ? s : 0.0;
  return m;
}
__device__ __forceinline__ int bin_of(u64 key, const BinMap& m) {
  const double t = (value_of(key) - m.vmin) * m.scale;   // NaN (inf * 0) compares false twice: bin 0
  return t >= (double)kQuantBins ? kQuantBins - 1 : (t > 0.0 ? (int)t : 0);
}

// the sum of v over the workgroup's 256 lanes, in every lane; sm [4]
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();   // the previous round's readers are done with sm
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// The passes over the source share one mapping: workgroup = (column block cb, chunk ch); lane = column cb 64 + (tid & 63); the four
// wavefronts take the chunk's vectors in turn, so a wavefront reads 64 consecutive columns of one vector.
struct PassMap {
  int cb, lane, wv, w;
  long long b0, b1;
  bool active;
};
__device__ __forceinline__ PassMap pass_map(const QuantArgs& A) {
  PassMap m;
  const int ncb = (A.wn + kQuantCols - 1) / kQuantCols;
  m.cb = (int)(blockIdx.x % (unsigned)ncb);
  const long long ch = blockIdx.x / (unsigned)ncb;
  m.lane = threadIdx.x & 63;
  m.wv = threadIdx.x >> 6;
  m.w = m.cb * kQuantCols + m.lane;
  m.active = m.w < A.wn;
  m.b0 = ch * A.chunk;
  m.b1 = m.b0 + A.chunk < (long long)A.B ? m.b0 + A.chunk : (long long)A.B;
  return m;
}

__global__ __launch_bounds__(kQuantThreads) void quant_init_kernel(QuantArgs A) {
  const long long i = (long long)blockIdx.x * kQuantThreads + threadIdx.x;
  const long long ncol = (long long)((A.wn + kQuantCols - 1) / kQuantCols) * kQuantCols;
  if (i < ncol * kQuantBins) A.hist[i] = 0u;
  if (i < ncol) {
    QuantCol c;
    c.kmin = ~0ull; c.kmax = 0ull; c.n = 0u; c.pad = 0u;
    A.col[i] = c;
  }
  if (i < ncol * A.T) {
    QuantTarget t;
    t.ans = 0ull; t.rank = 0u; t.m = 0u; t.cnt = 0u; t.who = ~0u; t.bucket = -1; t.state = kQuantDone;
    A.tgt[i] = t;
  }
}

__global__ __launch_bounds__(kQuantThreads) void quant_range_kernel(QuantArgs A) {
  __shared__ u64 smin[kQuantThreads], smax[kQuantThreads];
  __shared__ uint32_t sn[kQuantThreads];
  const PassMap m = pass_map(A);
  u64 kmin = ~0ull, kmax = 0ull;
  uint32_t n = 0;
  if (m.active) {
    const u64* p = A.src + A.w0 + m.w;
#pragma unroll 4
    for (long long b = m.b0 + m.wv; b < m.b1; b += 4) {
      const u64 u = p[b * A.ld];
      if (finite_bits(u)) {
        const u64 k = key_of(u);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        n++;
      }
    }
  }
  smin[threadIdx.x] = kmin; smax[threadIdx.x] = kmax; sn[threadIdx.x] = n;
  __syncthreads();
  if (m.wv == 0 && m.active) {
    for (int v = 1; v < 4; v++) {
      const u64 a = smin[v * 64 + m.lane], b = smax[v * 64 + m.lane];
      kmin = a < kmin ? a : kmin;
      kmax = b > kmax ? b : kmax;
      n += sn[v * 64 + m.lane];
    }
    if (n) {
      atomicAdd(&A.col[m.w].n, n);
      atomicMin(&A.col[m.w].kmin, kmin);
      atomicMax(&A.col[m.w].kmax, kmax);
    }
  }
}

// 32-bit words of LDS hold two 16-bit counters (bins 2 i and 2 i + 1 of a column): a chunk has fewer than 65536 vectors, so a
// counter never carries into its neighbour.  Word (bin / 2) 64 + lane: the lanes of a wavefront hit 64 different banks.
__global__ __launch_bounds__(kQuantThreads) void quant_hist_kernel(QuantArgs A) {
  __shared__ uint32_t h[kQuantBins / 2 * kQuantCols];
  const PassMap m = pass_map(A);
  for (int i = threadIdx.x; i < kQuantBins / 2 * kQuantCols; i += kQuantThreads) h[i] = 0u;
  bool live = false;
  BinMap bm{0.0, 0.0};
  if (m.active) {
    const QuantCol c = A.col[m.w];
    live = c.n > 0 && c.kmin != c.kmax;   // an empty or constant column is settled by the range pass
    if (live) bm = bin_map(c.kmin, c.kmax);
  }
  if (!__syncthreads_or(live)) return;
  if (live) {
    const u64* p = A.src + A.w0 + m.w;
#pragma unroll 4
    for (long long b = m.b0 + m.wv; b < m.b1; b += 4) {
      const u64 u = p[b * A.ld];
      if (finite_bits(u)) {
        const int bin = bin_of(key_of(u), bm);
        atomicAdd(&h[(bin >> 1) * kQuantCols + m.lane], 1u << ((bin & 1) * 16));
      }
    }
  }
  __syncthreads();
  uint32_t* g = A.hist + (size_t)m.cb * kQuantBins * kQuantCols;
  for (int i = threadIdx.x; i < kQuantBins / 2 * kQuantCols; i += kQuantThreads) {
    const uint32_t v = h[i];
    const int pair = i >> 6, l = i & 63;
    if (v & 0xffffu) atomicAdd(&g[(2 * pair) * kQuantCols + l], v & 0xffffu);
    if (v >> 16) atomicAdd(&g[(2 * pair + 1) * kQuantCols + l], v >> 16);
  }
}

// where q and who of (slab column w, target t) go: [W][nq][2], t = 2 j + side
__device__ __forceinline__ size_t out_index(const QuantArgs& A, int w, int t) { return ((size_t)(A.w0 + w) * A.nq) * 2 + t; }

// one lane per (column, target), the column running fastest: count, the rank rule, and what settles the target
__global__ __launch_bounds__(kQuantThreads) void quant_locate_kernel(QuantArgs A) {
  const long long i = (long long)blockIdx.x * kQuantThreads + threadIdx.x;
  if (i >= (long long)A.wn * A.T) return;
  const int w = (int)(i % A.wn), t = (int)(i / A.wn);
  const QuantCol c = A.col[w];
  if (t == 0 && A.count) A.count[A.w0 + w] = (double)c.n;
  QuantTarget* T = &A.tgt[(size_t)w * A.T + t];
  const size_t o = out_index(A, w, t);
  if (c.n == 0) {
    A.q[o] = __longlong_as_double(0x7ff8000000000000ll);
    atomicAdd(&A.counters[1], 1ull);
    return;
  }
  const double hq = A.probs[t >> 1] * (double)(c.n - 1u);   // one product, one rounding
  const uint32_t r = (uint32_t)((t & 1) ? ceil(hq) : floor(hq));
  if (c.kmin == c.kmax) {
    T->ans = c.kmin;
    A.q[o] = value_of(c.kmin);
    atomicAdd(&A.counters[1], 1ull);
    return;
  }
  const uint32_t* g = A.hist + (size_t)(w / kQuantCols) * kQuantBins * kQuantCols + (w % kQuantCols);
  uint32_t cum = 0, cnt = 0;
  int bin = 0;
  for (; bin < kQuantBins; bin++) {
    cnt = g[bin * kQuantCols];
    if (r < cum + cnt) break;
    cum += cnt;
  }
  if (bin < kQuantBins && cnt <= (uint32_t)kQuantCap) {
    T->rank = r - cum; T->m = cnt; T->bucket = bin; T->state = kQuantCand;
    atomicAdd(&A.counters[2], 1ull);
  } else {   // (bin == kQuantBins cannot happen: the bins hold all n entries and r < n; it would go to the fallback too)
    T->rank = r; T->state = kQuantFallback;
    atomicAdd(&A.counters[3], 1ull);
  }
}

__global__ __launch_bounds__(kQuantThreads) void quant_gather_kernel(QuantArgs A) {
  __shared__ int16_t tb[2 * kQuantMaxQ * kQuantCols];        // [t][lane]: the bin target t of the lane's column wants, or -1
  __shared__ uint32_t mask[kQuantBins / 32 * kQuantCols];    // [word][lane]: the bins any target of the column wants
  const PassMap m = pass_map(A);
  for (int i = threadIdx.x; i < kQuantBins / 32 * kQuantCols; i += kQuantThreads) mask[i] = 0u;
  __syncthreads();
  bool any = false;
  for (int i = threadIdx.x; i < A.T * kQuantCols; i += kQuantThreads) {
    const int t = i >> 6, l = i & 63, w = m.cb * kQuantCols + l;
    int bucket = -1;
    if (w < A.wn) {
      const QuantTarget* T = &A.tgt[(size_t)w * A.T + t];
      if (T->state == kQuantCand) bucket = T->bucket;
    }
    tb[i] = (int16_t)bucket;
    if (bucket >= 0) {
      atomicOr(&mask[(bucket >> 5) * kQuantCols + l], 1u << (bucket & 31));
      any = true;
    }
  }
  if (!__syncthreads_or(any)) return;
  if (!m.active) return;
  const QuantCol c = A.col[m.w];
  if (c.n == 0 || c.kmin == c.kmax) return;
  const BinMap bm = bin_map(c.kmin, c.kmax);
  const u64* p = A.src + A.w0 + m.w;
  QuantTarget* T = &A.tgt[(size_t)m.w * A.T];
  u64* cand = A.cand + (size_t)m.w * A.T * kQuantCap;
#pragma unroll 2
  for (long long b = m.b0 + m.wv; b < m.b1; b += 4) {
    const u64 u = p[b * A.ld];
    if (!finite_bits(u)) continue;
    const u64 k = key_of(u);
    const int bin = bin_of(k, bm);
    if (!((mask[(bin >> 5) * kQuantCols + m.lane] >> (bin & 31)) & 1u)) continue;
    for (int t = 0; t < A.T; t++) {
      if (tb[t * kQuantCols + m.lane] != bin) continue;
      const uint32_t pos = atomicAdd(&T[t].cnt, 1u);
      if (pos < (uint32_t)kQuantCap) cand[(size_t)t * kQuantCap + pos] = k;   // (pos < m <= cap: the histogram counted these entries)
    }
  }
}

// The smallest key K in [lo, hi] with at least `need` counted keys <= K, by bisection; count(K) must be the same in every lane.
template <class Count>
__device__ __forceinline__ u64 bisect(u64 lo, u64 hi, uint32_t need, const Count& count) {
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (count(mid) >= need) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// one workgroup per target whose bucket fits the buffer: the keys into LDS, their range, bisection inside it
__global__ __launch_bounds__(kQuantThreads) void quant_select_kernel(QuantArgs A) {
  __shared__ u64 keys[kQuantCap];
  __shared__ u64 srange[2];
  __shared__ uint32_t sm[4];
  QuantTarget* T = &A.tgt[blockIdx.x];
  if (T->state != kQuantCand) return;
  const uint32_t mcnt = T->m < (uint32_t)kQuantCap ? T->m : (uint32_t)kQuantCap;
  const u64* cand = A.cand + (size_t)blockIdx.x * kQuantCap;
  if (threadIdx.x == 0) { srange[0] = ~0ull; srange[1] = 0ull; }
  __syncthreads();
  u64 kmin = ~0ull, kmax = 0ull;
  for (uint32_t i = threadIdx.x; i < mcnt; i += kQuantThreads) {
    const u64 k = cand[i];
    keys[i] = k;
    kmin = k < kmin ? k : kmin;
    kmax = k > kmax ? k : kmax;
  }
  if (threadIdx.x < mcnt) {
    atomicMin(&srange[0], kmin);
    atomicMax(&srange[1], kmax);
  }
  __syncthreads();
  const u64 ans = bisect(srange[0], srange[1], T->rank + 1u, [&](u64 pivot) {
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < mcnt; i += kQuantThreads) c += keys[i] <= pivot ? 1u : 0u;
    return block_sum(c, sm);
  });
  if (threadIdx.x == 0) {
    const int w = (int)(blockIdx.x / (unsigned)A.T), t = (int)(blockIdx.x % (unsigned)A.T);
    T->ans = ans;
    A.q[out_index(A, w, t)] = value_of(ans);
  }
}

// One workgroup per target that is still open: the key is found eight bits at a time, from the first byte in which the column's
// extremes differ downwards.  A round counts, over the whole column, the finite keys that carry the prefix found so far by their
// next byte (256 integer counters in LDS), and walks the counts to the byte that holds the rank: bisection with 256 pivots per
// round, at most 8 rounds over the column instead of 64.  Exits at once where the target is settled.
__global__ __launch_bounds__(kQuantThreads) void quant_fallback_kernel(QuantArgs A) {
  __shared__ uint32_t cnt[256];
  __shared__ uint32_t found[2];
  QuantTarget* T = &A.tgt[blockIdx.x];
  if (T->state != kQuantFallback) return;
  const int w = (int)(blockIdx.x / (unsigned)A.T), t = (int)(blockIdx.x % (unsigned)A.T);
  const QuantCol c = A.col[w];
  const u64* p = A.src + A.w0 + w;
  uint32_t rank = T->rank;
  const int top = 63 - __clzll((long long)(c.kmin ^ c.kmax));   // (kmin != kmax: a constant column never comes here)
  int shift = top & ~7;
  u64 prefix = shift < 56 ? c.kmin >> (shift + 8) : 0ull;       // the bytes above: those of every finite key of the column
  for (; shift >= 0; shift -= 8) {
    cnt[threadIdx.x] = 0u;   // (kQuantThreads = 256 counters)
    __syncthreads();
    // a column's entries lie ld doubles apart, one cache line each: eight loads in flight per lane hide some of that
    for (long long b0 = threadIdx.x; b0 < (long long)A.B; b0 += 8 * kQuantThreads) {
      u64 u[8];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const long long b = b0 + (long long)i * kQuantThreads;
        u[i] = b < (long long)A.B ? p[b * A.ld] : ~0ull;   // (all ones: a NaN, left out like one)
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const u64 k = key_of(u[i]);
        if (finite_bits(u[i]) && (shift == 56 || (k >> (shift + 8)) == prefix)) atomicAdd(&cnt[(uint32_t)(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t cum = 0;
      int byte = 0;
      for (; byte < 255; byte++) {
        const uint32_t n = cnt[byte];
        if (rank < cum + n) break;
        cum += n;
      }
      found[0] = (uint32_t)byte;
      found[1] = rank - cum;
    }
    __syncthreads();
    prefix = (prefix << 8) | found[0];
    rank = found[1];
  }
  if (threadIdx.x == 0) {
    T->ans = prefix;
    A.q[out_index(A, w, t)] = value_of(prefix);
  }
}

// the lowest vector whose key is a target's answer: integer minimum, first in the workgroup's LDS, then one atomic per hit target.
// A 64-bit filter per lane (one bit per answer of the column, by a multiplicative hash of the key) keeps most entries off the loop.
__device__ __forceinline__ u64 who_bit(u64 k) { return 1ull << ((k * 0x9e3779b97f4a7c15ull) >> 58); }
__global__ __launch_bounds__(kQuantThreads) void quant_who_kernel(QuantArgs A) {
  __shared__ u64 ans[2 * kQuantMaxQ * kQuantCols];        // [t][lane]
  __shared__ uint32_t first[2 * kQuantMaxQ * kQuantCols];
  const PassMap m = pass_map(A);
  for (int i = threadIdx.x; i < A.T * kQuantCols; i += kQuantThreads) {
    const int t = i >> 6, l = i & 63, w = m.cb * kQuantCols + l;
    ans[i] = w < A.wn ? A.tgt[(size_t)w * A.T + t].ans : 0ull;
    first[i] = ~0u;
  }
  __syncthreads();
  if (m.active && A.col[m.w].n > 0) {
    u64 filter = 0ull;
    for (int t = 0; t < A.T; t++) filter |= who_bit(ans[t * kQuantCols + m.lane]);
    const u64* p = A.src + A.w0 + m.w;
#pragma unroll 2
    for (long long b = m.b0 + m.wv; b < m.b1; b += 4) {
      const u64 u = p[b * A.ld];
      if (!finite_bits(u)) continue;
      const u64 k = key_of(u);
      if (!(filter & who_bit(k))) continue;
      for (int t = 0; t < A.T; t++)
        if (ans[t * kQuantCols + m.lane] == k) atomicMin(&first[t * kQuantCols + m.lane], (uint32_t)b);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < A.T * kQuantCols; i += kQuantThreads) {
    const int t = i >> 6, w = m.cb * kQuantCols + (i & 63);
    if (first[i] != ~0u) atomicMin(&A.tgt[(size_t)w * A.T + t].who, first[i]);
  }
}

__global__ __launch_bounds__(kQuantThreads) void quant_who_write_kernel(QuantArgs A) {
  const long long i = (long long)blockIdx.x * kQuantThreads + threadIdx.x;
  if (i >= (long long)A.wn * A.T) return;
  const int w = (int)(i % A.wn), t = (int)(i / A.wn);
  const uint32_t b = A.tgt[(size_t)w * A.T + t].who;
  A.who[out_index(A, w, t)] = b == ~0u ? -1.0 : (double)b;
}

}  // namespace

hipError_t launch_quant_slab(const QuantArgs& A, hipStream_t s) {
  if (A.wn <= 0) return hipSuccess;
  const long long ncb = (A.wn + kQuantCols - 1) / kQuantCols, ntgt = (long long)A.wn * A.T;
  const long long ninit = ncb * kQuantCols * (kQuantBins > A.T ? kQuantBins : A.T);
  const dim3 blk(kQuantThreads);
  const auto per_lane = [](long long n) { return dim3((unsigned)((n + kQuantThreads - 1) / kQuantThreads)); };
  const long long nchunks = A.B > 0 ? ((long long)A.B + A.chunk - 1) / A.chunk : 0;
  const dim3 pass((unsigned)(ncb * nchunks));
  hipLaunchKernelGGL(quant_init_kernel, per_lane(ninit), blk, 0, s, A);
  if (const hipError_t e = hipGetLastError()) return e;
  if (nchunks > 0) {
    hipLaunchKernelGGL(quant_range_kernel, pass, blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(quant_hist_kernel, pass, blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(quant_locate_kernel, per_lane(ntgt), blk, 0, s, A);
  if (const hipError_t e = hipGetLastError()) return e;
  if (nchunks > 0) {
    hipLaunchKernelGGL(quant_gather_kernel, pass, blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(quant_select_kernel, dim3((unsigned)ntgt), blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(quant_fallback_kernel, dim3((unsigned)ntgt), blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  if (A.who) {
    if (nchunks > 0) {
      hipLaunchKernelGGL(quant_who_kernel, pass, blk, 0, s, A);
      if (const hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(quant_who_write_kernel, per_lane(ntgt), blk, 0, s, A);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace gel
