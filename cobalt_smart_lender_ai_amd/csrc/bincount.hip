// Per-feature, per-bin, per-class weighted counts of a row-major float32 matrix in one pass (gfx950): the
// primitive under the drift reports (PSI / CSI) and the WoE / IV tables of monitor/drift.py, whose
// bin_counts_host is the definition. Integer accumulation only, so the table has the same bits in any order
// of the additions: no floating-point atomics, nothing to make deterministic.
//
// Layout. Feature f has K_f interior edges (finite, strictly increasing, checked by the caller) and K_f + 2
// cells; cell_ptr[f] is its first cell in the concatenated table (cell_ptr[F] = all cells), so its edges start
// at cell_ptr[f] - 2 f of `edges`. A value x goes to cell #{i : z[i] < x} (searchsorted "left": intervals
// (z[b-1], z[b]], -inf in cell 0, +inf in cell K_f) and NaN to the missing cell K_f + 1. counts is
// int64 [C, cells], C = 2 with labels (class = y > 0.5, NaN labels in class 0), else 1; the kernel adds to it.
//
// Design choices
//  * A feature group is a run of consecutive features whose cell_ptr entries, edges and 32-bit counters fit in
//    kBinLdsWords of LDS (63 KiB, under the 64 KiB a kernel gets without opting in); groups are filled
//    greedily by group_end, which the host (for gridDim.y and the LDS size) and the kernel (blockIdx.y -> its
//    features) both run on the same cell_ptr, so there is no plan to upload. The launch asks for the largest
//    group's bytes only: 20 features of 9 edges are 2.5 KiB and leave the occupancy to the registers.
//  * A block of 512 threads walks tiles of kBinTileRows = 2048 rows. The elements of a tile (rows x the group's
//    features, row-major) are taken kBinBlock apart, so a wave reads consecutive addresses of X and its 64
//    lanes spread over the group's features: on one-hot columns, where every row lands in one of two cells,
//    a cell sees width / 64 lanes of a wave instead of all of them. Four loads are issued before the first
//    search. Each lane binary-searches its feature's edges in LDS and does one integer LDS atomic add.
//  * Overflow of a 32-bit LDS counter: BOUNDED TILES, not an early flush. A weight is at most 2^20
//    (models.sketch.quantize_weights) and a tile has 2048 rows, so a counter reaches at most 2^31 between two
//    flushes when every row of the tile lands in one cell; with weights the block flushes after every tile.
//    Without weights a row adds 1, the block keeps its counters over all its tiles (at most 2^20 of them, 2^31
//    rows) and flushes once: a flush is one 64-bit global atomic per non-zero counter, and with 255 edges
//    and 20 features that is 10k atomics, a quarter of a tile's elements. A test inside the loop ("flush when
//    a counter is near the top") would cost a compare per element to save nothing the bound does not give.
//  * Blocks: at most kBinMaxBlocksX per group, each with a contiguous run of tiles, so the flushes per cell
//    stay at ~1024 however long the matrix is.
//  * Refusals come before any launch: -1 F < 1, -2 ldx < F, -3 n < 0, -4 counts is null, -5 a feature with
//    more than kBinMaxEdges edges (or a cell_ptr that does not start at 0 or gives a feature fewer than 2
//    cells), -6 another missing pointer, -7 more groups or blocks than a grid holds. n == 0 is a no-op.
#include "common.h"
#include <algorithm>
#include <limits.h>

using namespace cobalt;

namespace {
constexpr int kBinBlock = 512;
constexpr int kBinTileRows = 2048;
constexpr int kBinMaxEdges = 4096;    // per feature
constexpr int kBinLdsWords = 16128;   // 63 KiB
constexpr int kBinMaxBlocksX = 1024;  // per feature group
constexpr int kBinMaxGroups = 65535;  // gridDim.y
constexpr int kBinMaxTilesPerBlock = 1 << 20;
constexpr int kBinBatch = 4;          // loads in flight per lane
static_assert((int64_t)kBinTileRows << 20 < ((int64_t)1 << 32), "a tile of maximum weights must fit a counter");
static_assert(3 + kBinMaxEdges + 2 * (kBinMaxEdges + 2) <= kBinLdsWords, "the widest feature must fit alone");

// LDS words of the features [f0, f1): f1 - f0 + 1 cell_ptr entries, their edges, C counters per cell.
__host__ __device__ __forceinline__ int group_words(const int32_t* cp, int f0, int f1, int C) {
  const int cells = cp[f1] - cp[f0];
  return (f1 - f0 + 1) + (cells - 2 * (f1 - f0)) + C * cells;
}

// One past the last feature of the group that starts at f0 (at least one feature: the widest fits alone).
__host__ __device__ __forceinline__ int group_end(const int32_t* cp, int F, int C, int f0) {
  int f1 = f0 + 1;
  while (f1 < F && group_words(cp, f0, f1 + 1, C) <= kBinLdsWords) ++f1;
  return f1;
}

// #{i : z[i] < x} over z[0 .. K): searchsorted "left". The caller handles NaN.
__device__ __forceinline__ int edges_below(const float* z, int K, float x) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (z[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
}  // namespace

// Block (x, g): the tiles [x * tiles_per_block, (x + 1) * tiles_per_block) of the rows, the features of group g.
template <bool HAS_Y, bool HAS_W>
__global__ __launch_bounds__(kBinBlock) void k_bin_counts(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                          const float* __restrict__ edges,
                                                          const int32_t* __restrict__ cell_ptr,
                                                          const float* __restrict__ y,
                                                          const int32_t* __restrict__ wq,
                                                          unsigned long long* __restrict__ counts,
                                                          int tiles_per_block) {
  extern __shared__ uint32_t s_mem[];
  constexpr int C = HAS_Y ? 2 : 1;
  const int tid = threadIdx.x;
  int f0 = 0, f1 = group_end(cell_ptr, F, C, 0);  // block-uniform
  for (int g = 0; g < (int)blockIdx.y; ++g) {
    if (f1 >= F) return;  // a group the host did not count: never with the cell_ptr the host saw
    f0 = f1;
    f1 = group_end(cell_ptr, F, C, f0);
  }
  const int gw = f1 - f0;
  const int c0 = cell_ptr[f0];
  const int gcells = cell_ptr[f1] - c0;
  const int gedges = gcells - 2 * gw;
  const int64_t total = cell_ptr[F];
  int32_t* s_ptr = reinterpret_cast<int32_t*>(s_mem);         // [gw + 1] first cell of each feature, minus c0
  float* s_edges = reinterpret_cast<float*>(s_mem + gw + 1);  // [gedges]
  uint32_t* s_cnt = s_mem + gw + 1 + gedges;                  // [C][gcells]
  for (int i = tid; i <= gw; i += kBinBlock) s_ptr[i] = cell_ptr[f0 + i] - c0;
  for (int i = tid; i < gedges; i += kBinBlock) s_edges[i] = edges[c0 - 2 * f0 + i];
  for (int i = tid; i < C * gcells; i += kBinBlock) s_cnt[i] = 0u;
  __syncthreads();

  const int64_t ntiles = (n + kBinTileRows - 1) / kBinTileRows;
  const int64_t t_begin = (int64_t)blockIdx.x * tiles_per_block;
  const int64_t t_end = min(t_begin + tiles_per_block, ntiles);
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t r0 = t * kBinTileRows;
    const int rows = (int)min((int64_t)kBinTileRows, n - r0);
    const uint32_t ne = (uint32_t)rows * (uint32_t)gw;  // < 2^11 * 2^13
    const float* Xt = X + r0 * ldx + f0;
    for (uint32_t base = tid; base < ne; base += kBinBlock * kBinBatch) {
      float x[kBinBatch];
      uint32_t row[kBinBatch], col[kBinBatch];
#pragma unroll
      for (int k = 0; k < kBinBatch; ++k) {
        const uint32_t e = base + k * kBinBlock;
        row[k] = e / (uint32_t)gw;
        col[k] = e - row[k] * (uint32_t)gw;
        x[k] = e < ne ? Xt[(int64_t)row[k] * ldx + col[k]] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < kBinBatch; ++k) {
        if (base + k * kBinBlock < ne) {
          const int j = (int)col[k];
          const int first = s_ptr[j];
          const int K = s_ptr[j + 1] - first - 2;
          const float xv = x[k];
          const int cell = (xv != xv) ? K + 1 : edges_below(s_edges + (first - 2 * j), K, xv);
          int cls = 0;
          if constexpr (HAS_Y) cls = y[r0 + row[k]] > 0.5f ? 1 : 0;
          uint32_t w = 1u;
          if constexpr (HAS_W) w = (uint32_t)wq[r0 + row[k]];
          atomicAdd(&s_cnt[cls * gcells + first + cell], w);
        }
      }
    }
    if (HAS_W || t + 1 == t_end) {
      __syncthreads();
      for (int i = tid; i < C * gcells; i += kBinBlock) {
        const uint32_t v = s_cnt[i];
        if (v != 0u) {
          const int c = i >= gcells ? 1 : 0;
          atomicAdd(&counts[c * total + c0 + (i - c * gcells)], (unsigned long long)v);
          s_cnt[i] = 0u;
        }
      }
      __syncthreads();
    }
  }
}

COBALT_API int cobalt_bin_counts_tile_rows() { return kBinTileRows; }
COBALT_API int cobalt_bin_counts_max_edges() { return kBinMaxEdges; }
COBALT_API int cobalt_bin_counts_max_blocks() { return kBinMaxBlocksX; }

// The feature groups of a table (cell_ptr_host: int32 [F + 1] on the host) with `classes` = 1 or 2 count
// rows: their number (gridDim.y of the launch), or the refusal of cobalt_bin_counts (-1, -5, -6, -7).
// group_first, when given, receives the first feature of every group and F (at most F + 1 entries).
COBALT_API int cobalt_bin_counts_groups(const int32_t* cell_ptr_host, int F, int classes, int32_t* group_first) {
  if (F < 1) return -1;
  if (cell_ptr_host == nullptr || (classes != 1 && classes != 2)) return -6;
  if (cell_ptr_host[0] != 0) return -5;
  for (int f = 0; f < F; ++f) {
    const int64_t K = (int64_t)cell_ptr_host[f + 1] - cell_ptr_host[f] - 2;
    if (K < 0 || K > kBinMaxEdges) return -5;
  }
  int G = 0;
  for (int f0 = 0; f0 < F; ++G) {
    if (group_first) group_first[G] = f0;
    f0 = group_end(cell_ptr_host, F, classes, f0);
  }
  if (group_first) group_first[G] = F;
  return G > kBinMaxGroups ? -7 : G;
}

// X: float32 rows ldx >= F apart on the device. edges: all features' edges concatenated, cell_ptr: int32
// [F + 1], on the host (checked here) and the same on the device (read by the kernel). y: float32 [n] or
// null; wq: int32 [n] in [0, 2^20] or null (1 per row). counts: int64 [C, cell_ptr[F]], added to.
COBALT_API int cobalt_bin_counts(const float* X, int64_t n, int F, int64_t ldx, const float* edges,
                                 const int32_t* cell_ptr_host, const int32_t* cell_ptr, const float* y,
                                 const int32_t* wq, int64_t* counts, hipStream_t stream) {
  if (F < 1) return -1;
  if (ldx < F) return -2;
  if (n < 0) return -3;
  if (counts == nullptr) return -4;
  const int C = y ? 2 : 1;
  const int G = cobalt_bin_counts_groups(cell_ptr_host, F, C, nullptr);
  if (G < 0) return G;
  if (cell_ptr == nullptr || (edges == nullptr && cell_ptr_host[F] > 2 * F)) return -6;
  if (n == 0) return 0;
  if (X == nullptr) return -6;
  int words = 0;
  for (int f0 = 0; f0 < F;) {
    const int f1 = group_end(cell_ptr_host, F, C, f0);
    words = std::max(words, group_words(cell_ptr_host, f0, f1, C));
    f0 = f1;
  }
  const int64_t ntiles = (n + kBinTileRows - 1) / kBinTileRows;
  const int64_t tpb = std::min<int64_t>((ntiles + kBinMaxBlocksX - 1) / kBinMaxBlocksX, kBinMaxTilesPerBlock);
  const int64_t gx = (ntiles + tpb - 1) / tpb;
  if (gx > INT_MAX) return -7;
  const auto fn = y ? (wq ? k_bin_counts<true, true> : k_bin_counts<true, false>)
                    : (wq ? k_bin_counts<false, true> : k_bin_counts<false, false>);
  hipLaunchKernelGGL(fn, dim3((unsigned)gx, (unsigned)G), dim3(kBinBlock), (size_t)words * sizeof(uint32_t), stream, X,
                     n, F, ldx, edges, cell_ptr, y, wq, reinterpret_cast<unsigned long long*>(counts), (int)tpb);
  CK_LAUNCH();
  return 0;
}
