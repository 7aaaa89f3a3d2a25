// Poisson-bootstrap replicates of the rank and operating-point metrics (AUC / Gini, KS, TP / FP, optional fp64
// sums) of one sorted score vector (gfx950): the primitive under metrics/bootstrap.py, whose
// bootstrap_sums_host is the definition and whose bootstrap_sums_tiled_host is this file's decomposition on the
// host. Every rank metric of every replicate is a ratio of exact 64-bit integers, so the host and the device
// give the same bits; the fp64 sums are plain sequential adds in row order (tile by tile), no atomics anywhere.
//
// Input. One 32-bit word per SORTED row (ascending score, stable): the original row index in the low 28 bits,
// then the label bit (28), the group-start bit (29: first row of a run of equal scores; row 0 has it) and the
// predicted-positive bit (30: score > threshold). Optionally two fp64 term columns [2, n] in sorted order.
//
// Counts. Replicate b gives ORIGINAL row i the count #{k : u >= T[k]} with u = word (b & 3) of
// Philox4x32-10(counter (i, b >> 2, 0, 0), key (seed lo, seed hi)) and T the Poisson(1) CDF scaled to 2^32: one
// Philox call serves the four replicates a thread owns. The counts never depend on the sorted position, so
// two score vectors over the same rows see the same resample (the paired comparison rests on it).
//
// Design choices
//  * k_boot_tiles: blockIdx.x is a tile of kBootTileRows consecutive sorted rows, blockIdx.y a group of
//    kBootBlockReps replicates. The tile's words (and terms) are staged in LDS once; every lane then walks the
//    rows IN ORDER and reads the same word: the LDS read is a broadcast, the word goes to a scalar register and
//    the branches on its bits are uniform. What differs between lanes is the Philox counter only.
//  * A tile cannot see where its first group began or where its last one ends, so it emits a record per
//    replicate: head (rows before the first start; the whole tile when it has none), middle (the complete
//    groups between the first and the last start: Pm, Nm and Lm = sum pos_g (2 negbelow_g + neg_g) with
//    negbelow counted inside the middle), tail (from the last start on), TP, FP and the two fp64 sums. Records
//    are [tile][field][replicate]: a lane stores four consecutive int64, a wave 2 KiB in a row.
//  * In-tile counts are 32-bit: at most 12 copies of kBootTileRows rows (static_assert below); the records and
//    everything in the stitch are 64-bit.
//  * k_boot_stitch: one thread per replicate walks the tiles in order with the closed negatives Ncl and the
//    open group (op, on): head joins the open group; a tile with a start closes it (U2 += op (2 Ncl + on)),
//    adds the middle (Lm + 2 Pm Ncl) and opens the tail. Whether a tile has a start depends on the scores only:
//    block row 0 writes one flag per tile, shared by all replicates.
//  * KS needs P and N before any maximum can be taken, so it is a second row pass (k_boot_ks, launched only
//    when asked for) that recomputes the counts instead of storing B x n bytes of them: per tile the maximum
//    and minimum over the middle's group ends of the local lp N - ln P (0 included: the middle's start is the
//    head group's end). k_boot_ks_stitch adds the tile's offset cumP N - cumN P and takes
//    max(offset + max, -(offset + min)). The last group ends at P N - N P = 0.
//  * Bound: n <= 2^28 rows of at most 12 copies give P, N < 2^32 and 2 P N < 2^63, so every integer fits.
//  * Refusals come before any launch: -1 n < 1, -2 n > 2^28, -3 reps < 1 or more than a grid holds, -4 rep0
//    negative or no multiple of 4, -5 words, workspace or out_int missing, -6 workspace too small, -7 ld < reps,
//    -8 terms without out_f, -9 unknown flag bits.
#include "common.h"
#include <limits.h>

using namespace cobalt;

namespace {
constexpr int kBootTileRows = 2048;
constexpr int kBootBlock = 128;
constexpr int kBootRepsPerThread = 4;  // one Philox call
constexpr int kBootBlockReps = kBootBlock * kBootRepsPerThread;
constexpr int kBootStitchBlock = 64;
constexpr int64_t kBootMaxRows = (int64_t)1 << 28;
constexpr int kBootMaxCount = 12;
constexpr int kBootRecFields = 9;  // Ph Nh Pm Nm Lm Pt Nt TP FP
constexpr int kBootOutFields = 6;  // P N U2 KSn TP FP
constexpr int kBootMaxGroups = 65535;
constexpr uint32_t kIdxMask = (1u << 28) - 1u, kLabelBit = 1u << 28, kStartBit = 1u << 29, kPredBit = 1u << 30;
constexpr int kFlagKs = 1, kFlagUnit = 2;
static_assert((int64_t)kBootMaxCount * kBootTileRows < ((int64_t)1 << 16),
              "a tile's counts, and pos * (2 negbelow + neg) of them, must fit 32 bits");
static_assert(kBootMaxCount * kBootMaxRows < ((int64_t)1 << 32), "P and N must fit 32 bits");

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// floor(2^32 PoissonCDF(k; 1)), k = 0 .. 11
__device__ __forceinline__ uint32_t poisson1(uint32_t u) {
  return (u >= 0x5e2d58d8u) + (u >= 0xbc5ab1b1u) + (u >= 0xeb715e1du) + (u >= 0xfb239797u) + (u >= 0xff1025f5u) +
         (u >= 0xffd90f3bu) + (u >= 0xfffa8b71u) + (u >= 0xffff540cu) + (u >= 0xffffed1fu) + (u >= 0xfffffe21u) +
         (u >= 0xffffffd4u) + (u >= 0xfffffffcu);
}

// The counts of original row i in the four replicates 4 q .. 4 q + 3.
template <bool UNIT>
__device__ __forceinline__ void row_counts(uint32_t i, uint32_t q, uint32_t k0, uint32_t k1, uint32_t c[4]) {
  if constexpr (UNIT) {
    c[0] = c[1] = c[2] = c[3] = 1u;
  } else {
    uint32_t x0 = i, x1 = q, x2 = 0u, x3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const uint32_t h0 = __umulhi(kPhiloxM0, x0), l0 = kPhiloxM0 * x0;
      const uint32_t h1 = __umulhi(kPhiloxM1, x2), l1 = kPhiloxM1 * x2;
      x0 = h1 ^ x1 ^ k0;
      x1 = l1;
      x2 = h0 ^ x3 ^ k1;
      x3 = l0;
      k0 += kPhiloxW0;
      k1 += kPhiloxW1;
    }
    c[0] = poisson1(x0);
    c[1] = poisson1(x1);
    c[2] = poisson1(x2);
    c[3] = poisson1(x3);
  }
}

__device__ __forceinline__ void store4(int64_t* p, const uint64_t v[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = (int64_t)v[j];
}
__device__ __forceinline__ void store4(int64_t* p, const uint32_t v[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = (int64_t)v[j];
}
}  // namespace

// Block (t, g): tile t of the sorted rows, replicates [g * kBootBlockReps, ...) of this call; a thread owns four.
// recs: int64 [tiles][kBootRecFields][Bp], fs: double [tiles][2][Bp], Bp = reps rounded up to 4 (a thread
// stores all four of its replicates; those past reps land in the padding). flags: int32 [tiles], starts in the
// tile capped at 2.
template <bool TERMS, bool UNIT>
__global__ __launch_bounds__(kBootBlock) void k_boot_tiles(const uint32_t* __restrict__ words,
                                                           const double* __restrict__ terms, int64_t n, uint32_t q0,
                                                           int reps, uint32_t k0, uint32_t k1,
                                                           int64_t* __restrict__ recs, double* __restrict__ fs,
                                                           int32_t* __restrict__ flags, int64_t Bp) {
  __shared__ uint32_t s_w[kBootTileRows];
  __shared__ double s_t[TERMS ? 2 * kBootTileRows : 2];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t row0 = tile * kBootTileRows;
  const int rows = (int)min((int64_t)kBootTileRows, n - row0);
  for (int r = tid; r < rows; r += kBootBlock) {
    s_w[r] = words[row0 + r];
    if constexpr (TERMS) {
      s_t[2 * r] = terms[row0 + r];
      s_t[2 * r + 1] = terms[n + row0 + r];
    }
  }
  __syncthreads();
  const int r0 = (int)blockIdx.y * kBootBlockReps + tid * kBootRepsPerThread;
  if (r0 >= reps) return;
  const uint32_t q = q0 + (uint32_t)(r0 >> 2);

  uint32_t gp[4] = {0, 0, 0, 0}, gn[4] = {0, 0, 0, 0}, Ph[4] = {0, 0, 0, 0}, Nh[4] = {0, 0, 0, 0};
  uint32_t Pm[4] = {0, 0, 0, 0}, Nm[4] = {0, 0, 0, 0}, TP[4] = {0, 0, 0, 0}, FP[4] = {0, 0, 0, 0};
  uint64_t Lm[4] = {0, 0, 0, 0};
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  int nstart = 0;
  for (int r = 0; r < rows; ++r) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_w[r]);  // every lane reads the same word
    uint32_t c[4];
    row_counts<UNIT>(w & kIdxMask, q, k0, k1, c);
    if (w & kStartBit) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (nstart == 0) {
          Ph[j] = gp[j];
          Nh[j] = gn[j];
        } else {
          Lm[j] += (uint64_t)gp[j] * (uint64_t)(2u * Nm[j] + gn[j]);
          Pm[j] += gp[j];
          Nm[j] += gn[j];
        }
        gp[j] = 0u;
        gn[j] = 0u;
      }
      nstart = nstart < 2 ? nstart + 1 : 2;
    }
    if (w & kLabelBit) {
#pragma unroll
      for (int j = 0; j < 4; ++j) gp[j] += c[j];
      if (w & kPredBit) {
#pragma unroll
        for (int j = 0; j < 4; ++j) TP[j] += c[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) gn[j] += c[j];
      if (w & kPredBit) {
#pragma unroll
        for (int j = 0; j < 4; ++j) FP[j] += c[j];
      }
    }
    if constexpr (TERMS) {
      const double t0 = s_t[2 * r], t1 = s_t[2 * r + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double cd = (double)c[j];
        s0[j] += cd * t0;
        s1[j] += cd * t1;
      }
    }
  }
  if (nstart == 0) {  // no start: the whole tile is head
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      Ph[j] = gp[j];
      Nh[j] = gn[j];
      gp[j] = 0u;
      gn[j] = 0u;
    }
  }
  int64_t* rec = recs + tile * kBootRecFields * Bp + r0;
  store4(rec + 0 * Bp, Ph);
  store4(rec + 1 * Bp, Nh);
  store4(rec + 2 * Bp, Pm);
  store4(rec + 3 * Bp, Nm);
  store4(rec + 4 * Bp, Lm);
  store4(rec + 5 * Bp, gp);
  store4(rec + 6 * Bp, gn);
  store4(rec + 7 * Bp, TP);
  store4(rec + 8 * Bp, FP);
  if constexpr (TERMS) {
    double* f = fs + tile * 2 * Bp + r0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = s0[j];
      f[Bp + j] = s1[j];
    }
  }
  if (blockIdx.y == 0 && tid == 0) flags[tile] = nstart;
}

// One thread per replicate: the records of all tiles, in order, into out_int [kBootOutFields][ld] (KSn = 0 here)
// and out_f [2][ld].
__global__ __launch_bounds__(kBootStitchBlock) void k_boot_stitch(const int64_t* __restrict__ recs,
                                                                  const double* __restrict__ fs,
                                                                  const int32_t* __restrict__ flags, int64_t tiles,
                                                                  int reps, int64_t Bp, int64_t* __restrict__ out_int,
                                                                  double* __restrict__ out_f, int64_t ld) {
  const int r = blockIdx.x * kBootStitchBlock + threadIdx.x;
  if (r >= reps) return;
  int64_t Ncl = 0, op = 0, on = 0, U2 = 0, P = 0, N = 0, TP = 0, FP = 0;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t* rec = recs + t * kBootRecFields * Bp + r;
    const int64_t Ph = rec[0], Nh = rec[Bp], Pm = rec[2 * Bp], Nm = rec[3 * Bp], Lm = rec[4 * Bp];
    const int64_t Pt = rec[5 * Bp], Nt = rec[6 * Bp];
    op += Ph;
    on += Nh;
    if (flags[t]) {
      U2 += op * (2 * Ncl + on);
      Ncl += on;
      U2 += Lm + 2 * Pm * Ncl;
      Ncl += Nm;
      op = Pt;
      on = Nt;
    }
    P += Ph + Pm + Pt;
    N += Nh + Nm + Nt;
    TP += rec[7 * Bp];
    FP += rec[8 * Bp];
    if (fs) {
      s0 += fs[t * 2 * Bp + r];
      s1 += fs[(t * 2 + 1) * Bp + r];
    }
  }
  U2 += op * (2 * Ncl + on);
  out_int[0 * ld + r] = P;
  out_int[1 * ld + r] = N;
  out_int[2 * ld + r] = U2;
  out_int[3 * ld + r] = 0;
  out_int[4 * ld + r] = TP;
  out_int[5 * ld + r] = FP;
  if (fs) {
    out_f[r] = s0;
    out_f[ld + r] = s1;
  }
}

// The second row pass: per (tile, replicate) the maximum and the minimum of lp N - ln P over the ends of the
// middle's groups, lp / ln counted from the tile's first start, 0 (the start itself) included. ks: int64
// [tiles][2][Bp]. P and N are rows 0 and 1 of out_int, written by k_boot_stitch earlier on the stream.
template <bool UNIT>
__global__ __launch_bounds__(kBootBlock) void k_boot_ks(const uint32_t* __restrict__ words, int64_t n, uint32_t q0,
                                                        int reps, uint32_t k0, uint32_t k1,
                                                        const int64_t* __restrict__ out_int, int64_t ld,
                                                        int64_t* __restrict__ ks, int64_t Bp) {
  __shared__ uint32_t s_w[kBootTileRows];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t row0 = tile * kBootTileRows;
  const int rows = (int)min((int64_t)kBootTileRows, n - row0);
  for (int r = tid; r < rows; r += kBootBlock) s_w[r] = words[row0 + r];
  __syncthreads();
  const int r0 = (int)blockIdx.y * kBootBlockReps + tid * kBootRepsPerThread;
  if (r0 >= reps) return;
  const uint32_t q = q0 + (uint32_t)(r0 >> 2);
  uint32_t P[4], N[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool live = r0 + j < reps;  // out_int has no padding
    P[j] = live ? (uint32_t)out_int[r0 + j] : 0u;
    N[j] = live ? (uint32_t)out_int[ld + r0 + j] : 0u;
  }
  uint32_t lp[4] = {0, 0, 0, 0}, ln[4] = {0, 0, 0, 0};
  int64_t mx[4] = {0, 0, 0, 0}, mn[4] = {0, 0, 0, 0};
  bool started = false;
  for (int r = 0; r < rows; ++r) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_w[r]);
    if (w & kStartBit) {
      if (started) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t d = (int64_t)((uint64_t)lp[j] * N[j]) - (int64_t)((uint64_t)ln[j] * P[j]);
          mx[j] = d > mx[j] ? d : mx[j];
          mn[j] = d < mn[j] ? d : mn[j];
        }
      }
      started = true;
    }
    if (!started) continue;  // the head: its counts are in the records already
    uint32_t c[4];
    row_counts<UNIT>(w & kIdxMask, q, k0, k1, c);
    if (w & kLabelBit) {
#pragma unroll
      for (int j = 0; j < 4; ++j) lp[j] += c[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) ln[j] += c[j];
    }
  }
  int64_t* k = ks + tile * 2 * Bp + r0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[j] = mx[j];
    k[Bp + j] = mn[j];
  }
}

// One thread per replicate: KSn = max over the group ends of |cumP N - cumN P| into row 3 of out_int.
__global__ __launch_bounds__(kBootStitchBlock) void k_boot_ks_stitch(const int64_t* __restrict__ recs,
                                                                     const int64_t* __restrict__ ks,
                                                                     const int32_t* __restrict__ flags,
                                                                     int64_t tiles, int reps, int64_t Bp,
                                                                     int64_t* __restrict__ out_int, int64_t ld) {
  const int r = blockIdx.x * kBootStitchBlock + threadIdx.x;
  if (r >= reps) return;
  const int64_t P = out_int[r], N = out_int[ld + r];
  int64_t cp = 0, cn = 0, best = 0;
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t* rec = recs + t * kBootRecFields * Bp + r;
    cp += rec[0];
    cn += rec[Bp];
    if (flags[t]) {
      const int64_t off = cp * N - cn * P;  // the open group ends where the tile's first start is
      const int64_t hi = off + ks[t * 2 * Bp + r], lo = -(off + ks[(t * 2 + 1) * Bp + r]);
      best = hi > best ? hi : best;
      best = lo > best ? lo : best;
      cp += rec[2 * Bp] + rec[5 * Bp];
      cn += rec[3 * Bp] + rec[6 * Bp];
    }
  }
  out_int[3 * ld + r] = best;
}

COBALT_API int cobalt_bootstrap_tile_rows() { return kBootTileRows; }
COBALT_API int cobalt_bootstrap_block_reps() { return kBootBlockReps; }
COBALT_API int cobalt_bootstrap_out_fields() { return kBootOutFields; }
COBALT_API int64_t cobalt_bootstrap_max_rows() { return kBootMaxRows; }

// Bytes of workspace for n rows and reps replicates in one call (with_terms / with_ks: non-zero when the fp64
// sums / the KS pass are wanted), or the refusal of cobalt_bootstrap for these shapes.
COBALT_API int64_t cobalt_bootstrap_workspace_bytes(int64_t n, int reps, int with_terms, int with_ks) {
  if (n < 1) return -1;
  if (n > kBootMaxRows) return -2;
  if (reps < 1 || (reps + kBootBlockReps - 1) / kBootBlockReps > kBootMaxGroups) return -3;
  const int64_t tiles = (n + kBootTileRows - 1) / kBootTileRows;
  const int64_t Bp = ((int64_t)reps + 3) / 4 * 4;
  const int64_t per_tile = (kBootRecFields + (with_terms ? 2 : 0) + (with_ks ? 2 : 0)) * Bp * 8;
  return tiles * per_tile + (tiles * 4 + 7) / 8 * 8;
}

// words: uint32 [n] (layout above); terms: double [2, n] in sorted order or null. Replicates rep0 .. rep0 + reps
// - 1 (rep0 a multiple of 4) go to columns 0 .. reps - 1 of out_int (int64 [6, ld]: P N U2 KSn TP FP) and out_f
// (double [2, ld], with terms only). flags: 1 = the KS pass (KSn is 0 without it), 2 = every count is 1 (the
// point estimate; seed unused). Everything runs on `stream`; workspace is scratch of at least
// cobalt_bootstrap_workspace_bytes and may be reused by the next call on the same stream.
COBALT_API int cobalt_bootstrap(const uint32_t* words, const double* terms, int64_t n, int64_t rep0, int reps,
                                uint64_t seed, int flags, void* workspace, int64_t workspace_bytes, int64_t* out_int,
                                double* out_f, int64_t ld, hipStream_t stream) {
  const bool with_ks = (flags & kFlagKs) != 0, unit = (flags & kFlagUnit) != 0;
  const int64_t need = cobalt_bootstrap_workspace_bytes(n, reps, terms != nullptr, with_ks);
  if (need < 0) return (int)need;
  if (rep0 < 0 || (rep0 & 3) != 0 || rep0 + reps > ((int64_t)1 << 32)) return -4;
  if (words == nullptr || workspace == nullptr || out_int == nullptr) return -5;
  if (workspace_bytes < need) return -6;
  if (ld < reps) return -7;
  if (terms != nullptr && out_f == nullptr) return -8;
  if (flags & ~(kFlagKs | kFlagUnit)) return -9;
  const int64_t tiles = (n + kBootTileRows - 1) / kBootTileRows;
  const int64_t Bp = ((int64_t)reps + 3) / 4 * 4;
  int64_t* recs = static_cast<int64_t*>(workspace);
  double* fs = terms ? reinterpret_cast<double*>(recs + tiles * kBootRecFields * Bp) : nullptr;
  int64_t* ks = recs + tiles * (kBootRecFields + (terms ? 2 : 0)) * Bp;
  int32_t* tile_flags = reinterpret_cast<int32_t*>(ks + (with_ks ? tiles * 2 * Bp : 0));
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32), q0 = (uint32_t)(rep0 >> 2);
  const dim3 grid((unsigned)tiles, (unsigned)((reps + kBootBlockReps - 1) / kBootBlockReps));
  const dim3 sgrid((unsigned)((reps + kBootStitchBlock - 1) / kBootStitchBlock));
  const auto tiles_fn = terms ? (unit ? k_boot_tiles<true, true> : k_boot_tiles<true, false>)
                              : (unit ? k_boot_tiles<false, true> : k_boot_tiles<false, false>);
  hipLaunchKernelGGL(tiles_fn, grid, dim3(kBootBlock), 0, stream, words, terms, n, q0, reps, k0, k1, recs, fs,
                     tile_flags, Bp);
  CK_LAUNCH();
  hipLaunchKernelGGL(k_boot_stitch, sgrid, dim3(kBootStitchBlock), 0, stream, recs, fs, tile_flags, tiles, reps, Bp,
                     out_int, out_f, ld);
  CK_LAUNCH();
  if (with_ks) {
    hipLaunchKernelGGL(unit ? k_boot_ks<true> : k_boot_ks<false>, grid, dim3(kBootBlock), 0, stream, words, n, q0,
                       reps, k0, k1, out_int, ld, ks, Bp);
    CK_LAUNCH();
    hipLaunchKernelGGL(k_boot_ks_stitch, sgrid, dim3(kBootStitchBlock), 0, stream, recs, ks, tile_flags, tiles, reps,
                       Bp, out_int, ld);
    CK_LAUNCH();
  }
  return 0;
}
