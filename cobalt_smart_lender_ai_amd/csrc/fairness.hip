// Poisson-bootstrap replicates of the fair-lending sums (gfx950): per replicate, protected group and cutoff the
// count-weighted number of rows, of bads, of declined rows and of declined bads, and the first two moments of the
// score on a 16-bit grid. The primitive under fairness/, whose fairness_sums_host is the definition and whose
// fairness_sums_tiled_host is this file's decomposition on the host. Every sum is a 64-bit integer added in a
// fixed order, no atomics anywhere, so the host and the device give the same bits.
//
// Input. One 8-byte record per row (uint2): x is the ORIGINAL row index in the low 28 bits, the label bit (28) and
// the padding bit (29: the row counts for nothing); y is the decline mask over the K cutoffs in its low 16 bits
// (bit k: score > cutoff k) and q = min(floor(score 65536), 65535) in its high 16 bits. As bytes: a uint32 word,
// a uint16 mask, a uint16 q.
//
// Counts. Replicate b gives ORIGINAL row i the count of bootstrap.hip (philox.h: counter (i, b >> 2, 0, 0), key
// (seed lo, seed hi), word b & 3, Poisson(1) thresholds): metrics.bootstrap_ci and this file see the same
// resample, whatever the order of the records. One Philox call serves the four replicates a thread owns.
//
// Fields, F = 4 + 2 K of them: n, B, S1, S2, D[0 .. K), DB[0 .. K) (sum of c, c y, c q, c q^2, c declined_k,
// c declined_k y).
//
// Design choices
//  * k_fair_tiles: blockIdx.x is a tile of kFairTileRows consecutive records, blockIdx.y a group of kFairBlockReps
//    replicates. The tile's records are staged in LDS once (16 KiB); every lane then walks them IN ORDER and reads
//    the same record with one 8-byte read: a broadcast, the record goes to scalar registers and every branch on
//    its bits (padding, label, the mask's bits) is uniform. What differs between lanes is the Philox counter.
//  * One form, no split of K over blockIdx.z: a split would repeat the Philox call and the twelve compares of
//    every count, which are most of a row's work, once per slice. What keeps the registers down instead: a tile
//    adds at most 12 kFairTileRows < 2^16 copies, so n, B, D_k and DB_k are 16-bit in the tile and the counter
//    of all rows shares a register with the counter of the bad rows (low and high half). A row adds
//    c * (bad ? 0x10001 : 1), a uniform factor, once per set mask bit. The kernel is specialised on the number
//    of mask bits it keeps counters for (1, 4 or 16). The compiler reports 34, 46 and 94 VGPRs for them (8, 8
//    and 5 waves per SIMD), no AGPRs, no scratch, and 16 KiB of LDS a block; with every count 1 (the point
//    estimate) the whole loop is scalar and takes 12 VGPRs.
//  * S1 is 32-bit in the tile (12 kFairTileRows 65535 < 2^32), S2 adds c q^2 with q^2 < 2^32 in 64 bits; the
//    static_asserts below hold the three bounds. Records are [tile][field][replicate] in 64 bits: a lane stores
//    four consecutive int64. Without labels the label bit is masked off where it is read, so B and DB are zeros.
//  * Groups: the caller sorts the records by group and pads every group to whole tiles with padding records, so a
//    tile belongs to one group. k_fair_stitch, one thread per (field, group, replicate), adds the tiles
//    tile_group[g] .. tile_group[g + 1] in order; an empty group gets zeros written.
//  * Bound: n <= 2^27 records of at most 12 copies give S2 <= 12 2^27 2^32 < 2^63.
//  * Refusals come before any launch: -1 n < 1, -2 n > 2^27, -3 reps < 1 or > 2^20, -4 rep0 negative or no
//    multiple of 4, -5 a null pointer, -6 workspace too small, -7 ld < reps, -8 K outside 1 .. 16, -9 G outside
//    1 .. 64, -10 unknown flag bits, -11 tile_group is not a non-decreasing table from 0 to the number of tiles.
#include "common.h"
#include "philox.h"

using namespace cobalt;

namespace {
constexpr int kFairTileRows = 2048;
constexpr int kFairBlock = 256;
constexpr int kFairRepsPerThread = 4;  // one Philox call
constexpr int kFairBlockReps = kFairBlock * kFairRepsPerThread;
constexpr int kFairStitchBlock = 256;
constexpr int64_t kFairMaxRows = (int64_t)1 << 27;
constexpr int kFairMaxReps = 1 << 20;
constexpr int kFairMaxCutoffs = 16;
constexpr int kFairMaxGroups = 64;
constexpr int kFairFixedFields = 4;  // n B S1 S2
constexpr uint32_t kFairIdxMask = (1u << 28) - 1u, kFairLabelBit = 1u << 28, kFairPadBit = 1u << 29;
constexpr uint32_t kFairQMax = 65535u;
constexpr int kFlagLabels = 1, kFlagUnit = 2;
static_assert((int64_t)kPoisson1MaxCount * kFairTileRows < ((int64_t)1 << 16),
              "a tile's n, B, D and DB must fit 16 bits: two of them share a register");
static_assert((int64_t)kPoisson1MaxCount * kFairTileRows * kFairQMax < ((int64_t)1 << 32),
              "a tile's S1 must fit 32 bits");
static_assert((int64_t)kFairQMax * kFairQMax < ((int64_t)1 << 32), "q^2 must fit 32 bits");
static_assert(kPoisson1MaxCount < 16 && kFairMaxRows == ((int64_t)1 << 27), "S2 <= 12 * 2^27 * 2^32 < 2^63");

struct FairGroupTable {
  int32_t first[kFairMaxGroups + 1];  // group g owns tiles first[g] .. first[g + 1]
};
}  // namespace

// Block (t, g): tile t of the records, replicates [g * kFairBlockReps, ...) of this call; a thread owns four.
// recs: int64 [tiles][4 + 2 K][Bp], Bp = reps rounded up to 4 (a thread stores all four of its replicates; those
// past reps land in the padding). KT: the mask bits with counters, K <= KT.
template <int KT, bool UNIT>
__global__ __launch_bounds__(kFairBlock) void k_fair_tiles(const uint2* __restrict__ rows_in, int64_t n, int K,
                                                           int labels, uint32_t q0, int reps, uint32_t k0,
                                                           uint32_t k1, int64_t* __restrict__ recs, int64_t Bp) {
  __shared__ uint2 s_rec[kFairTileRows];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t row0 = tile * kFairTileRows;
  const int rows = (int)min((int64_t)kFairTileRows, n - row0);
  for (int r = tid; r < rows; r += kFairBlock) s_rec[r] = rows_in[row0 + r];
  __syncthreads();
  const int r0 = (int)blockIdx.y * kFairBlockReps + tid * kFairRepsPerThread;
  if (r0 >= reps) return;
  const uint32_t q = q0 + (uint32_t)(r0 >> 2);

  // nb and dd hold two 16-bit counters each: all rows in the low half, the bad rows in the high half
  uint32_t nb[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  uint64_t s2[4] = {0, 0, 0, 0};
  uint32_t dd[KT][4];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dd[k][j] = 0u;
  }
  for (int r = 0; r < rows; ++r) {
    const uint2 rec = s_rec[r];  // every lane reads the same record
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x);
    const uint32_t mq = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.y);
    if (w & kFairPadBit) continue;
    uint32_t c[4];
    if constexpr (UNIT) {
      c[0] = c[1] = c[2] = c[3] = 1u;
    } else {
      bootstrap_row_counts(w & kFairIdxMask, q, k0, k1, c);
    }
    const uint32_t qv = mq >> 16, qq = qv * qv, mask = mq & 0xffffu;
    const uint32_t both = labels && (w & kFairLabelBit) ? 0x10001u : 1u;
    uint32_t cc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cc[j] = c[j] * both;
      nb[j] += cc[j];
      s1[j] += c[j] * qv;
      s2[j] += (uint64_t)c[j] * qq;
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (mask & (1u << k)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) dd[k][j] += cc[j];
      }
    }
  }
  const int F = kFairFixedFields + 2 * K;
  int64_t* rec = recs + tile * F * Bp + r0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rec[0 * Bp + j] = (int64_t)(nb[j] & 0xffffu);
    rec[1 * Bp + j] = (int64_t)(nb[j] >> 16);
    rec[2 * Bp + j] = (int64_t)s1[j];
    rec[3 * Bp + j] = (int64_t)s2[j];
  }
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k < K) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        rec[(kFairFixedFields + k) * Bp + j] = (int64_t)(dd[k][j] & 0xffffu);
        rec[(kFairFixedFields + K + k) * Bp + j] = (int64_t)(dd[k][j] >> 16);
      }
    }
  }
}

// One thread per (field, group, replicate): the records of the group's tiles, in order, into out [F][G][ld].
__global__ __launch_bounds__(kFairStitchBlock) void k_fair_stitch(const int64_t* __restrict__ recs,
                                                                  FairGroupTable grp, int G, int K, int reps,
                                                                  int64_t Bp, int64_t* __restrict__ out,
                                                                  int64_t ld) {
  const int r = blockIdx.x * kFairStitchBlock + threadIdx.x;
  const int g = blockIdx.y, f = blockIdx.z;
  if (r >= reps) return;
  const int F = kFairFixedFields + 2 * K;
  int64_t sum = 0;
  for (int64_t t = grp.first[g]; t < grp.first[g + 1]; ++t) sum += recs[(t * F + f) * Bp + r];
  out[((int64_t)f * G + g) * ld + r] = sum;
}

COBALT_API int cobalt_fairness_tile_rows() { return kFairTileRows; }
COBALT_API int cobalt_fairness_block_reps() { return kFairBlockReps; }
COBALT_API int64_t cobalt_fairness_max_rows() { return kFairMaxRows; }

// Bytes of workspace for n records, reps replicates and K cutoffs in one call, or the refusal of cobalt_fairness
// for these shapes.
COBALT_API int64_t cobalt_fairness_workspace_bytes(int64_t n, int reps, int K) {
  if (n < 1) return -1;
  if (n > kFairMaxRows) return -2;
  if (reps < 1 || reps > kFairMaxReps) return -3;
  if (K < 1 || K > kFairMaxCutoffs) return -8;
  const int64_t tiles = (n + kFairTileRows - 1) / kFairTileRows;
  const int64_t Bp = ((int64_t)reps + 3) / 4 * 4;
  return tiles * (kFairFixedFields + 2 * K) * Bp * 8;
}

// rows: uint2 [n] (layout above), sorted by group and padded so that every tile belongs to one group; tile_group:
// HOST int32 [G + 1], group g owns tiles tile_group[g] .. tile_group[g + 1] (tile_group[G] is the number of
// tiles). Replicates rep0 .. rep0 + reps - 1 (rep0 a multiple of 4) go to columns 0 .. reps - 1 of out (int64
// [4 + 2 K, G, ld]). flags: 1 = the label bits count (without it B and DB are zeros), 2 = every count is 1 (the
// point estimate; seed unused). Everything runs on `stream`; workspace is scratch of at least
// cobalt_fairness_workspace_bytes and may be reused by the next call on the same stream.
COBALT_API int cobalt_fairness(const void* rows, int64_t n, int K, const int32_t* tile_group, int G, int64_t rep0,
                               int reps, uint64_t seed, int flags, void* workspace, int64_t workspace_bytes,
                               int64_t* out, int64_t ld, hipStream_t stream) {
  const int64_t need = cobalt_fairness_workspace_bytes(n, reps, K);
  if (need < 0) return (int)need;
  if (rep0 < 0 || (rep0 & 3) != 0 || rep0 + reps > ((int64_t)1 << 32)) return -4;
  if (rows == nullptr || tile_group == nullptr || workspace == nullptr || out == nullptr) return -5;
  if (workspace_bytes < need) return -6;
  if (ld < reps) return -7;
  if (G < 1 || G > kFairMaxGroups) return -9;
  if (flags & ~(kFlagLabels | kFlagUnit)) return -10;
  const int64_t tiles = (n + kFairTileRows - 1) / kFairTileRows;
  FairGroupTable grp;
  for (int g = 0; g <= kFairMaxGroups; ++g) grp.first[g] = tile_group[g < G ? g : G];
  if (grp.first[0] != 0 || grp.first[G] != tiles) return -11;
  for (int g = 0; g < G; ++g)
    if (grp.first[g + 1] < grp.first[g]) return -11;
  const bool labels = (flags & kFlagLabels) != 0, unit = (flags & kFlagUnit) != 0;
  const int64_t Bp = ((int64_t)reps + 3) / 4 * 4;
  int64_t* recs = static_cast<int64_t*>(workspace);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32), q0 = (uint32_t)(rep0 >> 2);
  const dim3 grid((unsigned)tiles, (unsigned)((reps + kFairBlockReps - 1) / kFairBlockReps));
  const dim3 sgrid((unsigned)((reps + kFairStitchBlock - 1) / kFairStitchBlock), (unsigned)G,
                   (unsigned)(kFairFixedFields + 2 * K));
  using TilesFn = void (*)(const uint2*, int64_t, int, int, uint32_t, int, uint32_t, uint32_t, int64_t*, int64_t);
  static const TilesFn kTiles[3][2] = {{k_fair_tiles<1, false>, k_fair_tiles<1, true>},
                                       {k_fair_tiles<4, false>, k_fair_tiles<4, true>},
                                       {k_fair_tiles<16, false>, k_fair_tiles<16, true>}};
  const TilesFn tiles_fn = kTiles[K <= 1 ? 0 : (K <= 4 ? 1 : 2)][unit ? 1 : 0];
  hipLaunchKernelGGL(tiles_fn, grid, dim3(kFairBlock), 0, stream, static_cast<const uint2*>(rows), n, K,
                     labels ? 1 : 0, q0, reps, k0, k1, recs, Bp);
  CK_LAUNCH();
  hipLaunchKernelGGL(k_fair_stitch, sgrid, dim3(kFairStitchBlock), 0, stream, recs, grp, G, K, reps, Bp, out, ld);
  CK_LAUNCH();
  return 0;
}
