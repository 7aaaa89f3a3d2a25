// Leaf indices of a tree ensemble (XGBoost's pred_leaf) and the refresh of a model's node statistics and
// leaf values on new labelled rows (XGBoost's process_type="update", updater="refresh") for gfx950.
//
// The packed forest, its tiles in LDS and the walk are those of the predictor: forest_walk.h.
//
// k_leaf_index     one thread per row (ForestBlock, walk_trees, as k_predict); walk_trees reports the leaf's
//                  index inside its tree and it is written tree-major: idx[tree - t0][row] uint16 (a packed
//                  tree has at most 65535 nodes).
// k_refresh_accum  one launch per tree, grid-stride over the rows: the margin takes the previous tree's new
//                  leaf value (looked up through that tree's index row), the row's gradient pair is computed
//                  in fp64 and quantised by the trainer's own quantiser for this tree (gbdt_math.h
//                  quantize_gh with subsample = 1, row key = row index), and (gq, hq) is added to the
//                  row's leaf cell of a per-block LDS table of int64 pairs; the table's non-zero cells go to
//                  global memory with 64-bit integer atomics. Integer sums: no order of additions changes them.
// k_refresh_finalize  one block per tree: every leaf adds its sums to its ancestors (parents recovered from
//                  the child fields; LDS integer atomics, so the internal sums are the exact sums of their
//                  two children whatever the order), then weight, cover and gain of every node in fp64 by the
//                  trainer's expressions (gbdt_math.h), the loss change of the internal nodes, and the tree's new leaf
//                  values for the next tree's accumulate pass.
// k_refresh_apply  adds a tree's leaf values to the margins (after the last tree of a group of trees).
// There are no floating-point atomics: the same input gives the same bits on every run and for every grouping
// of the trees.
#include "common.h"
#include "forest_walk.h"
#include "gbdt_math.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kLeafBlock = 256;
constexpr int kAccBlock = 256;
constexpr int kAccRowsPerThread = 8; // rows a thread takes before the grid is widened
constexpr int kAccMaxGrid = 2048;    // 8 blocks on each of the 256 CUs
constexpr int kFinBlock = 256;
constexpr uint32_t kLeaf = 0xFFFFu;

// The key of the trainer's dither draws for one tree (gbdt.hip computes it per tree on the device).
inline uint64_t dither_key(uint64_t seed, int tree) { return splitmix64(tree_key_of(seed, tree) ^ kDitherSalt); }
}  // namespace

// Trees [t0, t1) of the forest: idx[(t - t0) * n + row] = index of the row's leaf inside tree t.
__global__ __launch_bounds__(kLeafBlock) void k_leaf_index(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                           const uint2* __restrict__ nodes,
                                                           const int32_t* __restrict__ tree_ptr,
                                                           const int32_t* __restrict__ tile_ptr, int n_tiles, int t0,
                                                           int t1, uint16_t* __restrict__ idx, int tile_cap) {
  const ForestBlock<kLeafBlock> fb(tile_cap, F, n);
  fb.stage_rows<false>(X, F, ldx);
  for (int tile = 0; tile < n_tiles; ++tile) {
    // the part of the tile inside [t0, t1); the bounds are the same for every thread of the block
    const int t_begin = max(tile_ptr[tile], t0), t_end = min(tile_ptr[tile + 1], t1);
    if (t_begin >= t_end) continue;
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    if (fb.row >= n) continue;
    walk_trees(fb.s_nodes, tree_ptr, nbase, t_begin, t_end, fb.x(),
               [&](int t, float, uint32_t at) { idx[(int64_t)(t - t0) * n + fb.row] = (uint16_t)at; });
  }
}

// One tree. idx_prev (nullable): the previous tree's index row, leaf_prev its new leaf values; tab[n_nodes][2]
// int64 (g, h) sums of this tree in global memory, zero before the first launch on it.
__global__ __launch_bounds__(kAccBlock) void k_refresh_accum(
    float* __restrict__ margin, const uint16_t* __restrict__ idx_prev, const float* __restrict__ leaf_prev,
    const uint16_t* __restrict__ idx_cur, const float* __restrict__ y, const float* __restrict__ w, int64_t n,
    double gscale, double hscale, uint64_t dkey, int wide, unsigned long long* __restrict__ tab, int n_nodes) {
  extern __shared__ unsigned long long s_tab[];  // [n_nodes][2]
  for (int i = threadIdx.x; i < 2 * n_nodes; i += kAccBlock) s_tab[i] = 0ull;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kAccBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kAccBlock) {
    float mf = margin[i];
    if (idx_prev) {
      mf += leaf_prev[idx_prev[i]];
      margin[i] = mf;
    }
    const double mm = (double)mf;
    const double p = 1.0 / (1.0 + exp(-mm));
    const double yd = (double)y[i], wd = (double)w[i];
    const double g = (p - yd) * wd;
    const double h = fmax(p * (1.0 - p), 1e-16) * wd;
    int64_t gq, hq;
    quantize_gh(g, h, gscale, hscale, dkey, i, gq, hq, wide != 0);
    const int c = idx_cur[i];
    if (c < n_nodes) {  // (always: the index was written by k_leaf_index for this tree)
      if (gq != 0) atomicAdd(&s_tab[2 * c], (unsigned long long)gq);
      if (hq != 0) atomicAdd(&s_tab[2 * c + 1], (unsigned long long)hq);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * n_nodes; i += kAccBlock) {
    const unsigned long long v = s_tab[i];
    if (v != 0ull) atomicAdd(&tab[i], v);
  }
}

// One tree, one block. nodes: the tree's packed nodes; tab: its leaf sums (internal cells zero) -> all node
// sums; stat_w / stat_h / stat_l: base weight, cover and loss change of every node; leaf_val: the leaf values
// the margins take (new ones when refresh_leaf, else the model's).
__global__ __launch_bounds__(kFinBlock) void k_refresh_finalize(
    const uint2* __restrict__ nodes, int n_nodes, unsigned long long* __restrict__ tab, double ginv, double hinv,
    double eta, double lambda, double alpha, double mcw, int refresh_leaf, float* __restrict__ stat_w,
    float* __restrict__ stat_h, float* __restrict__ stat_l, float* __restrict__ leaf_val) {
  extern __shared__ unsigned long long s_fin[];  // [n_nodes][2] sums, [n_nodes] gains, [n_nodes] parents
  unsigned long long* s_sum = s_fin;
  double* s_gain = reinterpret_cast<double*>(s_fin + 2 * (size_t)n_nodes);
  uint16_t* s_par = reinterpret_cast<uint16_t*>(s_fin + 3 * (size_t)n_nodes);
  for (int j = threadIdx.x; j < n_nodes; j += kFinBlock) {
    s_sum[2 * j] = tab[2 * j];
    s_sum[2 * j + 1] = tab[2 * j + 1];
    const uint32_t l = nodes[j].x & kLeaf;
    if (l != kLeaf && l + 1 < (uint32_t)n_nodes) s_par[l] = s_par[l + 1] = (uint16_t)j;
    if (j == 0) s_par[0] = (uint16_t)kLeaf;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_nodes; j += kFinBlock) {
    if ((nodes[j].x & kLeaf) != kLeaf) continue;
    const unsigned long long g = s_sum[2 * j], h = s_sum[2 * j + 1];  // (a leaf's cells: nobody adds to them)
    if (g == 0ull && h == 0ull) continue;
    // BFS numbering: a parent's index is below its child's, so the walk ends at the root (parent 0xFFFF)
    for (uint32_t c = j, p = s_par[j]; p < c; c = p, p = s_par[c]) {
      if (g != 0ull) atomicAdd(&s_sum[2 * p], g);
      if (h != 0ull) atomicAdd(&s_sum[2 * p + 1], h);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_nodes; j += kFinBlock) {
    const long long gs = (long long)s_sum[2 * j], hs = (long long)s_sum[2 * j + 1];
    tab[2 * j] = (unsigned long long)gs;
    tab[2 * j + 1] = (unsigned long long)hs;
    const double G = (double)gs * ginv, H = (double)hs * hinv;
    const double wgt = calc_weight(G, H, lambda, alpha, mcw);
    s_gain[j] = calc_gain(G, H, lambda, alpha, mcw);
    stat_w[j] = (float)wgt;
    stat_h[j] = (float)H;
    const uint2 nd = nodes[j];
    leaf_val[j] = (nd.x & kLeaf) != kLeaf ? 0.0f : (refresh_leaf ? (float)(wgt * eta) : __uint_as_float(nd.y));
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_nodes; j += kFinBlock) {
    const uint32_t l = nodes[j].x & kLeaf;
    stat_l[j] = (l != kLeaf && l + 1 < (uint32_t)n_nodes) ? (float)((s_gain[l] + s_gain[l + 1]) - s_gain[j]) : 0.0f;
  }
}

__global__ __launch_bounds__(kAccBlock) void k_refresh_apply(float* __restrict__ margin,
                                                             const uint16_t* __restrict__ idx,
                                                             const float* __restrict__ leaf_val, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kAccBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kAccBlock)
    margin[i] += leaf_val[idx[i]];
}

static int leaf_index_launch(const float* X, int64_t n, int F, int64_t ldx, const uint2* nodes,
                             const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles, int tile_cap, int t0,
                             int t1, uint16_t* idx, hipStream_t stream) {
  if (const int rc = forest_limits(tile_cap, F, kLeafBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kLeafBlock);
  static size_t attr_set = kDefaultMaxLds;
  CK(raise_dynamic_lds((const void*)k_leaf_index, lds, attr_set));
  hipLaunchKernelGGL(k_leaf_index, dim3(ceil_div(n, kLeafBlock)), dim3(kLeafBlock), lds, stream, X, n, F, ldx, nodes,
                     tree_ptr, tile_ptr, n_tiles, t0, t1, idx, tile_cap);
  CK_LAUNCH();
  return 0;
}

// idx [t1 - t0, n] uint16: the packed index (inside its tree) of the leaf every row reaches in the trees
// [t0, t1) of the forest. Returns -2 / -3 for a tile or an LDS footprint outside the limits (as cobalt_predict),
// -4 for a tree range outside the forest; nothing is launched then.
COBALT_API int cobalt_leaf_index(const float* X, int64_t n, int F, int64_t ldx, const void* nodes,
                                 const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles, int tile_cap,
                                 int n_trees, int t0, int t1, uint16_t* idx, hipStream_t stream) {
  if (t0 < 0 || t1 > n_trees || t0 > t1) return -4;
  if (n <= 0 || t0 == t1) return 0;
  return leaf_index_launch(X, n, F, ldx, static_cast<const uint2*>(nodes), tree_ptr, tile_ptr, n_tiles, tile_cap, t0,
                           t1, idx, stream);
}

static int acc_grid(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kAccMaxGrid, (n + (int64_t)kAccBlock * kAccRowsPerThread - 1) /
                                                                        ((int64_t)kAccBlock * kAccRowsPerThread)));
}

// Largest tree (nodes) the refresh kernels take: the finalize block holds 26 bytes per node in LDS.
COBALT_API int cobalt_refresh_max_nodes() { return (int)(kMaxLds / 26); }

// Refresh on the rows (X, y, w): tree by tree, in tree order, all launches on `stream` without a host
// synchronisation. tree_ptr_host: the host copy of tree_ptr ([n_trees + 1]); margin [n]: in = the base margin,
// out = the margins of the refreshed model; idx: workspace [group_trees, n] uint16 (the trees are processed in
// groups of group_trees, each group's indices computed by one k_leaf_index launch); sums [M, 2] int64, stats
// [3, M] float32 (base weight, cover, loss change) and leaf_val [M] float32 per packed node (M = all nodes).
// Returns -2 / -3 (tile / LDS limits of the walk), -5 (a tree too large for the LDS tables), -6 (bad
// arguments); nothing is launched then.
COBALT_API int cobalt_refresh(const float* X, int64_t n, int F, int64_t ldx, const float* y, const float* w,
                              const void* nodes, const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles,
                              int tile_cap, int n_trees, const int32_t* tree_ptr_host, double eta, double lambda,
                              double alpha, double mcw, double gscale, double hscale, uint64_t seed, int grad_bits,
                              int refresh_leaf, int group_trees, uint16_t* idx, int64_t* sums, float* stats,
                              float* leaf_val, float* margin, hipStream_t stream) {
  if (n <= 0 || n_trees <= 0) return 0;
  if (group_trees < 1 || (grad_bits != 17 && grad_bits != 25) || !(gscale > 0.0) || !(hscale > 0.0) ||
      tree_ptr_host == nullptr || tree_ptr_host[0] != 0)
    return -6;
  if (const int rc = forest_limits(tile_cap, F, kLeafBlock)) return rc;
  int biggest = 0;
  for (int t = 0; t < n_trees; ++t) {
    const int nn = tree_ptr_host[t + 1] - tree_ptr_host[t];
    if (nn < 1 || nn > 0xFFFF) return -6;
    biggest = std::max(biggest, nn);
  }
  if (biggest > cobalt_refresh_max_nodes()) return -5;
  const size_t lds_acc = (size_t)biggest * 16, lds_fin = (size_t)biggest * 26;
  static size_t acc_set = kDefaultMaxLds, fin_set = kDefaultMaxLds;
  CK(raise_dynamic_lds((const void*)k_refresh_accum, lds_acc, acc_set));
  CK(raise_dynamic_lds((const void*)k_refresh_finalize, lds_fin, fin_set));
  const int64_t M = tree_ptr_host[n_trees];
  const uint2* nd = static_cast<const uint2*>(nodes);
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(sums);
  CK(hipMemsetAsync(sums, 0, (size_t)M * 2 * sizeof(int64_t), stream));
  const int grid = acc_grid(n);
  const double ginv = 1.0 / gscale, hinv = 1.0 / hscale;
  for (int g0 = 0; g0 < n_trees; g0 += group_trees) {
    const int g1 = std::min(n_trees, g0 + group_trees);
    const int rc = leaf_index_launch(X, n, F, ldx, nd, tree_ptr, tile_ptr, n_tiles, tile_cap, g0, g1, idx, stream);
    if (rc != 0) return rc;
    for (int t = g0; t < g1; ++t) {
      const int64_t nb = tree_ptr_host[t];
      const int nn = tree_ptr_host[t + 1] - tree_ptr_host[t];
      const uint16_t* cur = idx + (int64_t)(t - g0) * n;
      const uint16_t* prev = t > g0 ? cur - n : nullptr;  // (a group's first tree: the margins are up to date)
      const float* leaf_prev = t > g0 ? leaf_val + tree_ptr_host[t - 1] : nullptr;
      hipLaunchKernelGGL(k_refresh_accum, dim3(grid), dim3(kAccBlock), (size_t)nn * 16, stream, margin, prev,
                         leaf_prev, cur, y, w, n, gscale, hscale, dither_key(seed, t), grad_bits == 25 ? 1 : 0,
                         tab + 2 * nb, nn);
      CK_LAUNCH();
      hipLaunchKernelGGL(k_refresh_finalize, dim3(1), dim3(kFinBlock), (size_t)nn * 26, stream, nd + nb, nn,
                         tab + 2 * nb, ginv, hinv, eta, lambda, alpha, mcw, refresh_leaf, stats + nb, stats + M + nb,
                         stats + 2 * M + nb, leaf_val + nb);
      CK_LAUNCH();
    }
    hipLaunchKernelGGL(k_refresh_apply, dim3(grid), dim3(kAccBlock), 0, stream, margin,
                       idx + (int64_t)(g1 - 1 - g0) * n, leaf_val + tree_ptr_host[g1 - 1], n);
    CK_LAUNCH();
  }
  return 0;
}
