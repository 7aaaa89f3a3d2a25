// Counterfactual recourse scan of a tree ensemble (gfx950): for every row and every actionable feature, the
// nearest single-feature moves that bring the row's margin to a target, and the move with the lowest margin.
//
// Along one feature, the others fixed, a forest's margin is piecewise constant and changes only at that
// feature's split thresholds, so a table of candidate values (one per interval between thresholds, or an
// explicit grid) covers every value the feature can take. For row r and actionable a (feature f = feats[a],
// candidates cand_val[cand_ptr[a] .. cand_ptr[a + 1]) ascending, window [jlo, jhi] = win[a], direction dir[a]):
//   c   = (number of candidates <= x[f]) - 1: the row's own position, never a result (-1: below all of them)
//   m_j = the margin of r with x[f] replaced by candidate j: the bits of predict_margin on the substituted row
//   slot 0 "down": the largest j < c in the window with m_j <= target           (not when dir = +1)
//   slot 1 "up":   the smallest j > c in the window with m_j <= target          (not when dir = -1)
//   slot 2 "best": the j != c in the window that dir allows with the smallest m_j; ties go to the smaller
//                  |j - c|, then to the smaller j
// Results are idx[r][a][slot] (candidate index inside the feature's own segment) and margin[r][a][slot]; an
// empty result is idx = -1 with the margin bits 0x7FC00000. A NaN x[f] makes all three empty.
//
// A client of the packed-forest block of forest_walk.h and of the grid-point walk of pdp_walk.h, shaped like
// k_pdp (pdp.hip): blockIdx.x is a 256-row block, blockIdx.y the actionable feature; the block stages its
// rows once, then loops over its window in chunks of kCandChunk = 16 candidates: the chunk's values are the
// same in every lane (scalar registers; the chunk's tail repeats the window's last candidate and is ignored),
// every forest tile is staged and each tree is walked for the 16 points, leaves added in fp32 in tree order
// from base_margin (no "tree ignores f" shortcut: every tree is walked for every candidate).
// The three running results are folded in registers after each chunk, candidates in ascending order.
// Everything is per thread: no cross-lane sums, no atomics, the same input gives the same bits. Threads
// without a row, or with a NaN x[f], take part in the barriers and do not walk. Neither X nor the staged row
// is written.
#include "common.h"
#include "pdp_walk.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kRcBlock = 256;
constexpr int kCandChunk = 16;
constexpr int64_t kRcChunkRows = 1 << 17;
constexpr int kRcMaxFeatures = 65535;  // gridDim.y
constexpr uint32_t kEmptyBits = 0x7FC00000u;
}  // namespace

__global__ __launch_bounds__(kRcBlock) void k_recourse(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                       const uint2* __restrict__ nodes,
                                                       const int32_t* __restrict__ tree_ptr,
                                                       const int32_t* __restrict__ tile_ptr, int n_tiles,
                                                       float base_margin, const int32_t* __restrict__ feats,
                                                       const int32_t* __restrict__ cand_ptr,
                                                       const float* __restrict__ cand_val,
                                                       const int32_t* __restrict__ win,
                                                       const int32_t* __restrict__ dir, float target,
                                                       int32_t* __restrict__ idx, float* __restrict__ margin, int A,
                                                       int tile_cap) {
  const ForestBlock<kRcBlock> fb(tile_cap, F, n);
  const int64_t row = fb.row;
  const int a = blockIdx.y;
  const int f = feats[a];
  const int seg = cand_ptr[a];
  const float* cv = cand_val + seg;
  const int K = cand_ptr[a + 1] - seg;
  const int jlo = win[2 * a], jhi = win[2 * a + 1], d = dir[a];
  const bool valid = row < n;
  // the row's own position: one binary search per thread, on the value in X (the staged copy is not visible
  // before the first tile's barrier)
  int c = -1;
  bool walk = false;
  if (valid) {
    const float xv = X[row * ldx + f];
    walk = xv == xv;
    int lo = 0, hi = K;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cv[mid] <= xv) lo = mid + 1;
      else hi = mid;
    }
    c = lo - 1;
  }
  int dn_j = -1, up_j = -1, be_j = -1;
  float dn_m = __uint_as_float(kEmptyBits), up_m = dn_m, be_m = dn_m;
  if (jlo <= jhi) {  // the same in every thread of the block
    fb.stage_rows<false>(X, F, ldx);
    const float* x = fb.x();
    for (int k0 = jlo; k0 <= jhi; k0 += kCandChunk) {
      GridVec<kCandChunk> v, acc;
#pragma unroll
      for (int i = 0; i < kCandChunk; ++i) {
        v[i] = cv[min(k0 + i, jhi)];
        acc[i] = base_margin;
      }
      for (int tile = 0; tile < n_tiles; ++tile) {
        const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
        const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
        if (walk)
          for (int t = t_begin; t < t_end; ++t)
            walk_tree_grid<kCandChunk, false>(fb.s_nodes, (uint32_t)(tree_ptr[t] - nbase), x, f, -1, v, v, acc);
      }
      // selects, not branches: 16 divergent ifs kept 16 exec masks in scalar registers and spilled them
#pragma unroll
      for (int i = 0; i < kCandChunk; ++i) {
        const int j = k0 + i;
        const float m = acc[i];
        const bool below = j < c;
        const bool ok = walk & (j <= jhi) & (j != c) & (below ? d != 1 : d != -1);
        const bool hit = ok & (m <= target);
        const bool dn = hit & below;  // ascending j: the last one is the largest
        const bool up = hit & !below & (up_j < 0);
        // ascending j: at equal margin and equal distance the one already held has the smaller j
        const bool be = ok & ((be_j < 0) | (m < be_m) | ((m == be_m) & (abs(j - c) < abs(be_j - c))));
        dn_j = dn ? j : dn_j;
        dn_m = dn ? m : dn_m;
        up_j = up ? j : up_j;
        up_m = up ? m : up_m;
        be_j = be ? j : be_j;
        be_m = be ? m : be_m;
      }
    }
  }
  if (valid) {
    const int64_t o = (row * A + a) * 3;
    idx[o] = dn_j;
    idx[o + 1] = up_j;
    idx[o + 2] = be_j;
    margin[o] = dn_m;
    margin[o + 1] = up_m;
    margin[o + 2] = be_m;
  }
}

COBALT_API int cobalt_recourse_chunk() { return kCandChunk; }
COBALT_API int64_t cobalt_recourse_chunk_rows() { return kRcChunkRows; }

// feats / cand_ptr / win / dir: the A actionable features on the device (read by the kernel); the *_host
// copies of the same are what is checked here. cand_val: n_cand float32 on the device, ascending per
// feature (the caller checks the contents). idx / margin: [n, A, 3]. Returns -2 / -3 for a tile or an LDS
// footprint outside the limits (as cobalt_pdp) and -8 for anything else outside the limits: A outside
// [1, 65535], a feature outside [0, F), a null table, a candidate segment outside [0, n_cand], a non-empty
// window (jlo <= jhi) outside its segment, a direction outside {-1, 0, 1}; nothing is launched then.
COBALT_API int cobalt_recourse_scan(const float* X, int64_t n, int F, int64_t ldx, const void* nodes,
                                    const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles, int tile_cap,
                                    float base_margin, const int32_t* feats_host, const int32_t* cand_ptr_host,
                                    const int32_t* win_host, const int32_t* dir_host, const int32_t* feats,
                                    const int32_t* cand_ptr, const float* cand_val, int64_t n_cand,
                                    const int32_t* win, const int32_t* dir, int A, float target, int32_t* idx,
                                    float* margin, hipStream_t stream) {
  if (F < 1 || A < 1 || A > kRcMaxFeatures || n < 0 || ldx < F) return -8;
  if (feats_host == nullptr || cand_ptr_host == nullptr || win_host == nullptr || dir_host == nullptr) return -8;
  if (feats == nullptr || cand_ptr == nullptr || cand_val == nullptr || win == nullptr || dir == nullptr) return -8;
  if (cand_ptr_host[0] < 0 || (int64_t)cand_ptr_host[A] > n_cand) return -8;
  for (int a = 0; a < A; ++a) {
    const int K = cand_ptr_host[a + 1] - cand_ptr_host[a];
    const int jlo = win_host[2 * a], jhi = win_host[2 * a + 1];
    if (feats_host[a] < 0 || feats_host[a] >= F || K < 0) return -8;
    if (jlo <= jhi && (jlo < 0 || jhi >= K)) return -8;
    if (dir_host[a] < -1 || dir_host[a] > 1) return -8;
  }
  if (const int rc = forest_limits(tile_cap, F, kRcBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kRcBlock);
  if (n == 0) return 0;
  if (idx == nullptr || margin == nullptr) return -8;
  static size_t attr_set = kDefaultMaxLds;
  CK(raise_dynamic_lds((const void*)k_recourse, lds, attr_set));
  const uint2* nd = static_cast<const uint2*>(nodes);
  const dim3 block(kRcBlock);
  for (int64_t r0 = 0; r0 < n; r0 += kRcChunkRows) {
    const int64_t nc = std::min(kRcChunkRows, n - r0);
    const dim3 grid(ceil_div(nc, kRcBlock), A);
    hipLaunchKernelGGL(k_recourse, grid, block, lds, stream, X + r0 * ldx, nc, F, ldx, nd, tree_ptr, tile_ptr, n_tiles,
                       base_margin, feats, cand_ptr, cand_val, win, dir, target, idx + r0 * A * 3,
                       margin + r0 * A * 3, A, tile_cap);
    CK_LAUNCH();
  }
  return 0;
}
