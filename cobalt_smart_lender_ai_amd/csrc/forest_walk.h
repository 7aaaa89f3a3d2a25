// "A block scores its rows against tiles of the packed forest": the one home of what the forest kernels
// share (predict.hip, evalcurve.hip, pdp.hip, permimp.hip, ale.hip, refresh.hip k_leaf_index). Forest layout
// (ops/predict_ops.py pack_forest): BFS-numbered trees, 8-byte nodes
//   uint32 meta = left_child(16 bits, 0xFFFF = leaf) | feature(15 bits) << 16 | default_left << 31
//   float  val  = split threshold (x < val goes left) or leaf value
// grouped into tiles of <= tile_cap nodes. A block stages its rows in LDS once (ForestBlock::stage_rows)
// and every tile in turn (stage_tile); each thread walks its row through the tile's trees (walk_trees
// here, the grid-point walks of pdp_walk.h). The host half (forest_limits, raise_dynamic_lds) is what
// every entry point checks before such a launch.
#pragma once
#include "common.h"

// LDS tile capacity (nodes) is chosen per model by the host packer (ops/predict_ops.py
// pack_forest: 2048 unless one tree is larger) and passed to the launch. Small tiles keep the
// per-block LDS footprint low -> more resident blocks per CU, which is what bounds this
// latency-bound walk: 125M-row scoring went 490M (6144-node tiles) -> 810M rows/s (2048).
constexpr int kMaxTileNodes = 8192;
constexpr size_t kMaxLds = 160 * 1024;         // dynamic LDS a block may ask for
constexpr size_t kDefaultMaxLds = 64 * 1024;   // ... and what a kernel gets without raise_dynamic_lds

// A tree walk is a chain of dependent LDS reads (node -> feature value -> next node), so one
// thread walks kWalk trees at once: the kWalk chains' loads are independent and overlap. The leaf
// values are still added to the margin one tree at a time in tree order (same fp32 sum).
// kWalk is the default; COBALT_PRED_WALK=2|8 selects the other instantiations for sweeps.
constexpr int kWalk = 4;

// The trees [t_begin, t_end) of the staged tile for the row at x: leaf(t, value, at) for every tree in
// tree order, `at` = the leaf's index inside its tree. A callback that ignores `at` costs nothing.
template <int kWalk = ::kWalk, typename Leaf>
__device__ __forceinline__ void walk_trees(const uint2* s_nodes, const int32_t* __restrict__ tree_ptr, int nbase,
                                           int t_begin, int t_end, const float* x, Leaf&& leaf) {
  for (int t = t_begin; t < t_end; t += kWalk) {
    uint32_t base[kWalk], at[kWalk];
    uint2 nd[kWalk];
#pragma unroll
    for (int k = 0; k < kWalk; ++k) {  // past the range's end: walk tree t again, result unused
      base[k] = (uint32_t)(tree_ptr[t + k < t_end ? t + k : t] - nbase);
      at[k] = 0;
      nd[k] = s_nodes[base[k]];
    }
    bool more = true;
    while (more) {
      more = false;
#pragma unroll
      for (int k = 0; k < kWalk; ++k) {
        if ((nd[k].x & 0xFFFFu) != 0xFFFFu) {
          const int f = (nd[k].x >> 16) & 0x7FFF;
          const float v = x[f];
          const bool left = (v != v) ? ((nd[k].x >> 31) != 0) : (v < __uint_as_float(nd[k].y));
          at[k] = (nd[k].x & 0xFFFFu) + (left ? 0u : 1u);
          nd[k] = s_nodes[base[k] + at[k]];
          more = true;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kWalk; ++k)
      if (t + k < t_end) leaf(t + k, __uint_as_float(nd[k].y), at[k]);
  }
}

// The block's view of its rows and of the dynamic LDS: s_nodes[tile_cap] then s_x[block][F | 1] (the odd
// stride makes the per-thread reads conflict-free). One thread owns row `row`, which exists when row < n
// (the kernels test that where they need it: a flag computed here would be held in registers across the
// predictor's walk); x() is its staged row.
// kBlock is the kernel's constant block size; 0 reads blockDim.x wherever the size is used (the predictor).
template <int kBlock = 0>
struct ForestBlock {
  uint2* s_nodes;
  float* s_x;
  int xs, nrows;
  int64_t row0, row;

  static __device__ __forceinline__ auto block() {
    if constexpr (kBlock > 0) return kBlock;
    else return (unsigned)blockDim.x;
  }

  __device__ __forceinline__ ForestBlock(int tile_cap, int F, int64_t n) {
    extern __shared__ unsigned char smem[];
    s_nodes = reinterpret_cast<uint2*>(smem);
    s_x = reinterpret_cast<float*>(smem + (size_t)tile_cap * sizeof(uint2));
    xs = F | 1;
    row0 = (int64_t)blockIdx.x * block();
    row = row0 + threadIdx.x;
    nrows = (int)min((int64_t)block(), n - row0);
  }
  __device__ __forceinline__ const float* x() const { return s_x + threadIdx.x * xs; }

  // Stage the block's rows (coalesced over the contiguous [nrows][F] slab when ldx == F); no barrier: the
  // first stage_tile brings one. kZeroTail = false copies the nrows rows that exist and the threads
  // without a row must not walk (the predictor, the leaf index: nothing staged or walked beyond the
  // batch); true also fills the rows past n with zeros, so that every lane walks and takes part in the
  // wave sums (wave_total_f64 needs every lane active).
  template <bool kZeroTail>
  __device__ __forceinline__ void stage_rows(const float* X, int F, int64_t ldx) const {
    if constexpr (kZeroTail) {
      for (int e = threadIdx.x; e < block() * F; e += block()) {
        const int r = e / F, f = e - r * F;
        s_x[r * xs + f] = r < nrows ? X[(row0 + r) * ldx + f] : 0.0f;
      }
    } else {
      for (int e = threadIdx.x; e < nrows * F; e += block()) {
        const int r = e / F, f = e - r * F;
        s_x[r * xs + f] = X[(row0 + r) * ldx + f];
      }
    }
  }

  __device__ __forceinline__ void copy_nodes(const uint2* nodes, int nbase, int nn) const {
    for (int i = threadIdx.x; i < nn; i += block()) s_nodes[i] = nodes[nbase + i];
  }

  // The tile loop's step, called by every thread of the block: wait until nobody reads the previous tile,
  // copy the nodes of the trees [t_begin, t_end) (inside one tile) to s_nodes, wait for the copy (and, the
  // first time, for the staged rows). Returns the first node's index, walk_trees' nbase.
  __device__ __forceinline__ int stage_tile(const uint2* nodes, const int32_t* tree_ptr, int t_begin,
                                            int t_end) const {
    const int nbase = tree_ptr[t_begin];
    const int nn = tree_ptr[t_end] - nbase;  // <= tile_cap
    __syncthreads();
    copy_nodes(nodes, nbase, nn);
    __syncthreads();
    return nbase;
  }

  // stage_rows<false> and ONE tile behind a single barrier (the tile's bounds are read before the rows).
  __device__ __forceinline__ int stage_rows_and_tile(const float* X, int F, int64_t ldx, const uint2* nodes,
                                                     const int32_t* tree_ptr, int t_begin, int t_end) const {
    const int nbase = tree_ptr[t_begin];
    const int nn = tree_ptr[t_end] - nbase;
    stage_rows<false>(X, F, ldx);
    copy_nodes(nodes, nbase, nn);
    __syncthreads();
    return nbase;
  }
};

// ---------------------------------------------------------------------------------------- host
inline size_t forest_lds_bytes(int tile_cap, int F, int block) {
  return (size_t)tile_cap * sizeof(uint2) + (size_t)block * (F | 1) * sizeof(float);
}

// 0, or the code every forest entry point returns before any launch: -2 for a tile outside
// [1, kMaxTileNodes], -3 for an LDS footprint above kMaxLds.
inline int forest_limits(int tile_cap, int F, int block) {
  if (tile_cap < 1 || tile_cap > kMaxTileNodes) return -2;
  if (forest_lds_bytes(tile_cap, F, block) > kMaxLds) return -3;
  return 0;
}

// Let kernel `fn` be launched with `lds` bytes of dynamic LDS. `high` is the caller's per-kernel
// high-water mark (static, initially kDefaultMaxLds): the attribute is set only when it has to grow.
inline hipError_t raise_dynamic_lds(const void* fn, size_t lds, size_t& high) {
  if (lds <= high) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) high = lds;
  return e;
}
