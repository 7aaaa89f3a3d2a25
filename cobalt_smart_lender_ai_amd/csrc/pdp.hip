// Partial dependence (PD) and individual conditional expectation (ICE) of a tree ensemble for one or two
// features (gfx950): every row is scored at every grid point with x[f1] (and x[f2]) replaced by the grid
// point's value, and the margins / probabilities are averaged per grid point.
//
// A client of the packed-forest block of forest_walk.h (ForestBlock): one thread owns one row (features
// staged in LDS with the odd stride F | 1, rows past n as zeros), tiles of the
// forest are staged in LDS, leaf values are added in fp32 in tree order starting from base_margin. Grid point
// k = i1 * G2 + i2 scores x[f1] = g1[i1], x[f2] = g2[i2] (f2 = -1: 1-D, G2 = 1); a NaN grid value is the
// "feature missing" point and takes the trees' default directions. ice[k][r] has the bits of predict_margin
// on the substituted row. The substitution is a select on the value read from LDS (pdp_walk.h): neither X
// nor the staged row is written.
//
// Design choices
//  * Forest staging is amortised over kGridChunk = 16 grid points: blockIdx.y is the grid chunk, a block
//    stages its rows once and every forest tile once and walks each tree for its 16 points, one fp32
//    accumulator per point (16 VGPRs). A G-point grid stages the forest ceil(G / 16) times per row block
//    instead of G times, and reads X ceil(G / 16) times. The last chunk's points past G score the last grid
//    point again; nothing is written for them.
//  * The kWalk = 4 chains that overlap their dependent LDS reads are 4 grid points of one tree
//    (pdp_walk.h walk_tree_grid); the trees are visited in order, so each point's sum keeps the tree order.
//  * The grid values of a chunk are the same in every lane: they are loaded once per block, the first axis
//    into scalar registers (16 SGPRs). The kernel is instantiated for 1-D (one compare per split) and 2-D (two
//    compares; the second axis' 16 values are pinned to vector registers, since 32 SGPRs of grid values made
//    the compiler spill scalar registers).
//  * No "tree ignores f1 / f2" shortcut: it was not measured, so it is not there.
//  * PD sums: per grid point sum w m and sum w p with m the fp32 margin widened to double and
//    p = 1 / (1 + exp(-m)) in double; the 64 lanes of a wave are summed by a fixed DPP sequence, the wave's
//    pair goes to workspace[point][wave], and k_pair_reduce (wave_partials.h) adds a point's partials in a fixed order. No
//    floating-point atomics: the same input gives the same bits on every run. Rows past n in the last block
//    walk a row of zeros and enter the wave sums as the constant 0.0.
//  * Rows are processed in chunks of kPdpChunkRows = 2^17 (2048 wave partials per grid point, which bounds
//    the workspace: 32 KiB per grid point); chunk sums are added in chunk order.
#include "common.h"
#include "pdp_walk.h"
#include "wave_partials.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kPdpBlock = 256;
constexpr int kGridChunk = 16;
constexpr int64_t kPdpChunkRows = 1 << 17;
constexpr int kPdpMaxGrid = 1 << 16;  // grid points per call (gridDim.y = points / kGridChunk <= 4096)
}  // namespace

// Rows [0, n) of one row chunk (blockIdx.x) at the grid points [blockIdx.y * kGridChunk, + kGridChunk).
// `ice` (nullable) points at the chunk's first row of the [G, ice_ld] matrix. SUMS: every wave writes
// part[point][wave] = (sum w m, sum w p) (rows of `nparts` pairs) and the waves of grid chunk 0 write
// wpart[wave] = sum w.
template <bool SUMS, bool TWO>
__global__ __launch_bounds__(kPdpBlock) void k_pdp(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                   const float* __restrict__ w, const uint2* __restrict__ nodes,
                                                   const int32_t* __restrict__ tree_ptr,
                                                   const int32_t* __restrict__ tile_ptr, int n_tiles,
                                                   float base_margin, int f1, int f2, const float* __restrict__ g1,
                                                   const float* __restrict__ g2, int G2, int G,
                                                   float* __restrict__ ice, int64_t ice_ld, double* __restrict__ part,
                                                   double* __restrict__ wpart, int nparts, int tile_cap) {
  const ForestBlock<kPdpBlock> fb(tile_cap, F, n);
  const int64_t row = fb.row;
  const bool valid = row < n;
  fb.stage_rows<true>(X, F, ldx);
  // the chunk's grid values (block-uniform); points past G repeat the last one
  const int k0 = blockIdx.y * kGridChunk;
  GridVec<kGridChunk> v1, v2, acc;
#pragma unroll
  for (int j = 0; j < kGridChunk; ++j) {
    const int k = min(k0 + j, G - 1);
    const int i1 = k / G2, i2 = k - i1 * G2;
    v1[j] = g1[i1];
    float b = 0.0f;
    if constexpr (TWO) {
      b = g2[i2];
      asm("" : "+v"(b));  // second axis in vector registers: 2 x 16 scalar registers made the kernel spill SGPRs
    }
    v2[j] = b;
    acc[j] = base_margin;
  }
  const float* x = fb.x();
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    for (int t = t_begin; t < t_end; ++t)
      walk_tree_grid<kGridChunk, TWO>(fb.s_nodes, (uint32_t)(tree_ptr[t] - nbase), x, f1, f2, v1, v2, acc);
  }
  if (ice && valid) {
#pragma unroll
    for (int j = 0; j < kGridChunk; ++j)
      if (k0 + j < G) ice[(int64_t)(k0 + j) * ice_ld + row] = acc[j];
  }
  if constexpr (SUMS) {
    const int wave_g = blockIdx.x * (kPdpBlock / kWave) + wave_id();  // < nparts
    const double wv = valid ? (w ? (double)w[row] : 1.0) : 0.0;
    if (blockIdx.y == 0) {
      const double sw = wave_total_f64(wv);
      if (lane_id() == kWave - 1) wpart[wave_g] = sw;
    }
#pragma unroll
    for (int j = 0; j < kGridChunk; ++j) {
      const double m = (double)acc[j];
      const double p = 1.0 / (1.0 + exp(-m));
      const double sm = wave_total_f64(valid ? wv * m : 0.0);
      const double sp = wave_total_f64(valid ? wv * p : 0.0);
      if (lane_id() == kWave - 1 && k0 + j < G) {
        double* dst = part + ((int64_t)(k0 + j) * nparts + wave_g) * 2;
        dst[0] = sm;
        dst[1] = sp;
      }
    }
  }
}

static int64_t pdp_parts(int64_t n) { return wave_parts(n, kPdpChunkRows, kPdpBlock); }

COBALT_API int cobalt_pdp_grid_chunk() { return kGridChunk; }
COBALT_API int64_t cobalt_pdp_chunk_rows() { return kPdpChunkRows; }
COBALT_API int cobalt_pdp_max_grid() { return kPdpMaxGrid; }

// Bytes of `workspace` for n rows and G grid points: [G][parts][2] + [parts] doubles with parts = the
// waves of one row chunk.
COBALT_API int64_t cobalt_pdp_workspace(int64_t n, int G) {
  if (n <= 0 || G <= 0) return 0;
  return wave_partials_bytes(G, pdp_parts(n));
}

// ice: [G1 * G2, n] float32 margins or nullptr; sums: [2 G + 1] doubles (sum w m, sum w p per grid point,
// then sum w) or nullptr (w and workspace are not touched then). f2 = -1: 1-D (g2 unused, G2 must be 1).
// Returns -2 / -3 for a tile or an LDS footprint outside the limits (as cobalt_eval_curve), -7 when sums are
// asked for without workspace, -8 for features or grid sizes outside their ranges; nothing is launched then.
COBALT_API int cobalt_pdp(const float* X, int64_t n, int F, int64_t ldx, const void* nodes, const int32_t* tree_ptr,
                          const int32_t* tile_ptr, int n_tiles, int tile_cap, float base_margin, int f1, int f2,
                          const float* g1, int G1, const float* g2, int G2, const float* w, float* ice,
                          void* workspace, double* sums, hipStream_t stream) {
  if (F < 1 || f1 < 0 || f1 >= F || f2 < -1 || f2 >= F || f2 == f1 || g1 == nullptr || G1 < 1 || G2 < 1) return -8;
  if (f2 < 0 ? G2 != 1 : g2 == nullptr) return -8;
  if ((int64_t)G1 * G2 > kPdpMaxGrid) return -8;
  if (const int rc = forest_limits(tile_cap, F, kPdpBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kPdpBlock);
  const bool want_sums = sums != nullptr;
  if (want_sums && workspace == nullptr) return -7;
  if (n <= 0 || (ice == nullptr && !want_sums)) return 0;
  using Kernel = decltype(&k_pdp<false, false>);
  static const Kernel kernels[4] = {k_pdp<false, false>, k_pdp<false, true>, k_pdp<true, false>, k_pdp<true, true>};
  const int which = (want_sums ? 2 : 0) + (f2 >= 0 ? 1 : 0);
  const Kernel fn = kernels[which];
  static size_t attr_set[4] = {kDefaultMaxLds, kDefaultMaxLds, kDefaultMaxLds, kDefaultMaxLds};
  CK(raise_dynamic_lds((const void*)fn, lds, attr_set[which]));
  const uint2* nd = static_cast<const uint2*>(nodes);
  const int G = G1 * G2;
  const int nparts = (int)pdp_parts(n);
  double* part = want_sums ? static_cast<double*>(workspace) : nullptr;
  double* wpart = wave_wpart(part, G, nparts);
  const dim3 block(kPdpBlock);
  for (int64_t r0 = 0; r0 < n; r0 += kPdpChunkRows) {
    const int64_t nc = std::min(kPdpChunkRows, n - r0);
    const dim3 grid(ceil_div(nc, kPdpBlock), ceil_div(G, kGridChunk));
    hipLaunchKernelGGL(fn, grid, block, lds, stream, X + r0 * ldx, nc, F, ldx, (want_sums && w) ? w + r0 : nullptr, nd,
                       tree_ptr, tile_ptr, n_tiles, base_margin, f1, f2, g1, g2, G2, G, ice ? ice + r0 : nullptr, n,
                       part, wpart, nparts, tile_cap);
    CK_LAUNCH();
    if (want_sums) {
      hipLaunchKernelGGL(k_pair_reduce<>, dim3(G + 1), dim3(kReduceBlock), 0, stream, part, wpart, nparts,
                         (int)pdp_parts(nc), G, sums, r0 > 0 ? 1 : 0);
      CK_LAUNCH();
    }
  }
  return 0;
}
