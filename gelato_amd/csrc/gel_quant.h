// gel_quant.h -- exact batched quantiles over the vectors of a batch (gel_batch_quantiles*): what host and kernels
// share (gel_kernels_quant.hip).  Everything is integer work on the 64-bit keys of the entries; the only floating-point operations
// are the rank product p (n - 1) and the monotone bin map, neither of which decides a result by its rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gel {

constexpr int kQuantMaxQ = 16;         // probabilities per call (GEL_QUANT_MAXQ); a column has 2 nq targets (the lower and upper rank)
constexpr int kQuantBins = 256;        // bins of a column's histogram
constexpr int kQuantCap = 2048;        // keys a target's candidate buffer holds; a fuller bucket goes to the bisection over the column
constexpr int kQuantCols = 64;         // columns per workgroup: a wavefront reads 64 consecutive columns of one vector (512 bytes)
constexpr int kQuantThreads = 256;     // lanes per workgroup of every kernel here
constexpr int kQuantChunk = 1024;      // vectors per workgroup of the passes over the source ...
constexpr int kQuantChunkNarrow = 256; // ... and where the slab has fewer than kQuantNarrowBlocks column blocks
constexpr int kQuantNarrowBlocks = 16;
constexpr size_t kQuantWsCap = (size_t)256 << 20;   // bytes of workspace a call takes at most: wider sources are walked in slabs
constexpr int kQuantMaxChunks = 65535;              // a chunk's 16-bit LDS counters hold 65535: B / 65535 < 32769 vectors per chunk

enum { kQuantDone = 0, kQuantCand = 1, kQuantFallback = 2 };

// one (column, rank): 32 bytes
struct QuantTarget {
  unsigned long long ans;   // the key found (valid once the target is settled; meaningless where n = 0)
  uint32_t rank;            // the rank among the column's finite entries (kQuantFallback), inside the bucket (kQuantCand)
  uint32_t m;               // entries of the bucket (kQuantCand)
  uint32_t cnt;             // candidates gathered so far (the position counter)
  uint32_t who;             // lowest vector whose key is ans; ~0: none
  int32_t bucket;           // the bin that holds the rank (kQuantCand), else -1
  int32_t state;            // kQuant*
};
struct QuantCol {
  unsigned long long kmin, kmax;   // over the finite entries
  uint32_t n, pad;
};

// the sections of the workspace for `cols` columns of T targets each, every one at a multiple of 256 bytes
struct QuantLayout {
  size_t counters, col, hist, tgt, cand, bytes;
};
inline size_t quant_up(size_t n, size_t a) { return (n + a - 1) / a * a; }
inline QuantLayout quant_layout(int64_t cols, int T) {
  QuantLayout L;
  const size_t c = (size_t)quant_up((size_t)cols, kQuantCols);   // whole column blocks: the histogram is [block][bin][64]
  L.counters = 0;
  L.col = 256;
  L.hist = L.col + quant_up(c * sizeof(QuantCol), 256);
  L.tgt = L.hist + quant_up(c * kQuantBins * sizeof(uint32_t), 256);
  L.cand = L.tgt + quant_up(c * T * sizeof(QuantTarget), 256);
  L.bytes = L.cand + c * T * (size_t)kQuantCap * sizeof(unsigned long long);
  return L;
}
// columns per slab: the most (a multiple of 64, at least 64) whose workspace stays within the cap
inline int64_t quant_slab_cols(int T) {
  int64_t s = kQuantCols;
  while (quant_layout(s + kQuantCols, T).bytes <= kQuantWsCap) s += kQuantCols;
  return s;
}
// vectors per workgroup of the passes over the source, for a slab of `cols` columns
inline int64_t quant_chunk(int64_t B, int64_t cols) {
  int64_t c = (cols + kQuantCols - 1) / kQuantCols < kQuantNarrowBlocks ? kQuantChunkNarrow : kQuantChunk;
  const int64_t least = ((B + kQuantMaxChunks - 1) / kQuantMaxChunks + 3) / 4 * 4;
  return c > least ? c : least;
}

struct QuantArgs {
  int32_t B, nq, T, chunk;
  int32_t wn, pad;             // columns of this slab
  int64_t ld, w0;              // leading dimension of the source; first column of the slab
  const unsigned long long* src;   // [B][ld], the entries' bits
  double probs[kQuantMaxQ];
  double* q;                   // [W][nq][2]
  double* count;               // [W] or null
  double* who;                 // [W][nq][2] or null
  unsigned long long* counters;    // [4]: targets, settled by the range pass, by the candidates, by the fallback (of the whole call)
  QuantCol* col;
  uint32_t* hist;              // [column block][bin][64]
  QuantTarget* tgt;            // [wn][T]
  unsigned long long* cand;    // [wn][T][kQuantCap]
};

// every launch of one slab on the stream s: init, range, histogram, locate, gather, select, fallback and, where A.who is given, the
// two kernels of the who pass.  A.B = 0: only init and locate run (the n = 0 pattern).
hipError_t launch_quant_slab(const QuantArgs& A, hipStream_t s);

}  // namespace gel
