// gel_comom.h -- batched co-moments over the vectors of a batch (gel_batch_comoments*): what host and kernels share
// (gel_kernels_comom.hip).  The order of every floating-point operation is stated in include/gelato_amd.h; nothing here may change it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gel {

constexpr int kComBlock = 256;     // vectors per partial: block k = vectors 256 k .. 256 k + 255 (the envelope's blocks)
constexpr int kComTileA = 32;      // a columns per workgroup of comom_block_kernel
constexpr int kComTileB = 32;      // b columns per workgroup
constexpr int kComRows = 64;       // counted rows staged in LDS at a time
constexpr int kComThreads = 256;   // lanes per workgroup: 16 x 16 lanes of 2 x 2 pairs each
constexpr size_t kComWsCap = (size_t)256 << 20;   // bytes of workspace a call takes at most: wider products are walked in slabs

inline size_t com_up(size_t n, size_t a) { return (n + a - 1) / a * a; }

// the sections of the workspace, every one at a multiple of 256 bytes.  Fixed part: per block the count and the first excluded
// vector, per vector the mask byte, per (block, a column) mean and m2; behind it, for one slab of an a columns by bn b columns, per
// (block, b column of the slab) mean and m2 and the pair partials [block][an][bn]
struct ComLayout {
  size_t info, cnt, fe, mask, sa, sb, cp, bytes;
};
inline ComLayout com_layout(int64_t B, int64_t Wa, int64_t an, int64_t bn) {
  const size_t nblk = (size_t)((B + kComBlock - 1) / kComBlock);
  ComLayout L;
  L.info = 0;
  L.cnt = 256;
  L.fe = L.cnt + com_up(nblk * sizeof(int32_t), 256);
  L.mask = L.fe + com_up(nblk * sizeof(int32_t), 256);
  L.sa = L.mask + com_up((size_t)B, 256);
  L.sb = L.sa + com_up(nblk * (size_t)Wa * 2 * sizeof(double), 256);
  L.cp = L.sb + com_up(nblk * (size_t)bn * 2 * sizeof(double), 256);
  L.bytes = L.cp + nblk * (size_t)an * (size_t)bn * sizeof(double);
  return L;
}

// the slab walk of a call: an a columns by bn b columns at a time, both whole tiles unless the view is narrower.  All a columns at
// once where one tile of b columns then fits the cap, else as many tiles of a as do; then as many tiles of b as fit beside them.
// max_a, max_b: upper limits on an, bn (GEL_COMOM_SLAB_ROWS, GEL_COMOM_SLAB; 0 = none).  ok = false: not even one tile of pairs fits
// beside the fixed part.
struct ComSlabs {
  int64_t an, bn;
  bool ok;
};
inline ComSlabs com_slabs(int64_t B, int64_t Wa, int64_t Wb, int64_t max_a, int64_t max_b) {
  ComSlabs S{0, 0, true};
  if (Wa <= 0 || Wb <= 0) return S;
  const size_t nblk = (size_t)((B + kComBlock - 1) / kComBlock);
  const size_t fixed = com_layout(B, Wa, 0, 0).bytes + 256;   // (the b statistics' section is rounded up to 256 bytes)
  const size_t room = fixed < kComWsCap ? (kComWsCap - fixed) / sizeof(double) : 0;   // doubles of the slab's part
  const size_t per = nblk ? nblk : 1;
  const int64_t tb = Wb < kComTileB ? Wb : kComTileB;
  int64_t an = Wa;                                               // a b column of the slab takes an + 2 doubles per block
  if ((size_t)(an + 2) * (size_t)tb * per > room) {
    const int64_t fit = (int64_t)(room / per / (size_t)tb) - 2;
    an = fit / kComTileA * kComTileA;
    if (an < kComTileA) { S.ok = false; return S; }
  }
  if (max_a > 0 && max_a < an) an = max_a;
  int64_t bn = (int64_t)(room / per / (size_t)(an + 2));
  if (bn >= Wb) bn = Wb;
  else bn = bn / kComTileB * kComTileB;
  if (max_b > 0 && max_b < bn) bn = max_b;
  if (bn < 1) { S.ok = false; return S; }
  S.an = an; S.bn = bn;
  return S;
}

struct ComArgs {
  int32_t B, self;
  int64_t Wa, inca, lda, Wb, incb, ldb;
  const double* a;
  const double* b;           // the self form: b = a, Wb = Wa, incb = inca, ldb = lda
  double* C;                 // [Wa][Wb]
  double* stat_a;            // [Wa][2] or null
  double* stat_b;            // [Wb][2] or null
  double* info;              // [2]
  // workspace
  int32_t* cnt;              // [blocks] counted vectors of the block
  int32_t* fe;               // [blocks] lowest excluded vector of the block, or INT32_MAX
  unsigned char* mask;       // [B] 1 = counted
  double* sa;                // [blocks][Wa][2] mean, m2
  double* sb;                // [blocks][bn][2] of the slab's b columns
  double* cp;                // [blocks][an][bn]
};

// the mask pass (one read of both views) and info
hipError_t launch_comom_mask(const ComArgs& A, hipStream_t s);
// one slab: the pairs (i, j), a0 <= i < a0 + an, b0 <= j < b0 + bn: block partials, then their merge into C
hipError_t launch_comom_slab(const ComArgs& A, int64_t a0, int64_t an, int64_t b0, int64_t bn, hipStream_t s);
// mean and m2 of W columns out of the blocks' statistics part [blocks][W][2] (A.sa; A.sb of the slab just walked) into out [W][2]
hipError_t launch_comom_stats(const ComArgs& A, int64_t W, const double* part, double* out, hipStream_t s);

}  // namespace gel
