// The packed-forest walk of the partial-dependence kernel (pdp.hip): the sibling of forest_walk.h
// walk_trees for a row that is scored at several grid points. Same nodes, same test
// (x < val goes left, NaN takes the default direction); the difference is where x comes from: at a split
// on f1 (TWO: or f2) the grid point's value replaces the row's, every other feature is read from the staged row. The staged row is never written.
#pragma once
#include "common.h"
#include "forest_walk.h"

// One float per grid point of a chunk, as a vector value: with constant indices (J below is a template
// argument) it lives in registers; a float array passed by reference was kept in scratch by the compiler.
template <int kChunk>
using GridVec = float __attribute__((ext_vector_type(kChunk)));

// kWalk grid points (J .. J + kWalk - 1 of the chunk) of one tree: kWalk independent chains whose LDS reads
// overlap (walk_trees: kWalk consecutive trees of one row). Every index into v1 / v2 / acc is a constant.
template <int J, int kChunk, int kWalk, bool TWO>
__device__ __forceinline__ void walk_tree_points(const uint2* s_nodes, uint32_t base, uint2 root, const float* x,
                                                 int f1, int f2, const GridVec<kChunk> v1, const GridVec<kChunk> v2,
                                                 GridVec<kChunk>& acc) {
  uint2 nd[kWalk];
#pragma unroll
  for (int k = 0; k < kWalk; ++k) nd[k] = root;
  bool more = true;
  while (more) {
    more = false;
#pragma unroll
    for (int k = 0; k < kWalk; ++k) {
      if ((nd[k].x & 0xFFFFu) != 0xFFFFu) {
        const int f = (nd[k].x >> 16) & 0x7FFF;
        const float xv = x[f];
        float v = f == f1 ? v1[J + k] : xv;
        if constexpr (TWO) v = f == f2 ? v2[J + k] : v;
        const bool left = (v != v) ? ((nd[k].x >> 31) != 0) : (v < __uint_as_float(nd[k].y));
        nd[k] = s_nodes[base + (nd[k].x & 0xFFFFu) + (left ? 0u : 1u)];
        more = true;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kWalk; ++k) acc[J + k] += __uint_as_float(nd[k].y);
}

// One tree, kChunk grid points, in groups of kWalk. acc[j] receives the leaf of grid point j; the caller
// visits the trees in order, so every acc[j] is the fp32 sum in tree order. v1 / v2 (v2 is unused without TWO) are the same in every
// lane (they depend on the block's grid chunk only): scalar registers.
template <int kChunk, bool TWO, int kWalk = ::kWalk, int J = 0>
__device__ __forceinline__ void walk_tree_grid(const uint2* s_nodes, uint32_t base, const float* x, int f1, int f2,
                                               const GridVec<kChunk> v1, const GridVec<kChunk> v2,
                                               GridVec<kChunk>& acc) {
  static_assert(kChunk % kWalk == 0, "the grid chunk is walked in groups of kWalk points");
  if constexpr (J < kChunk) {
    walk_tree_points<J, kChunk, kWalk, TWO>(s_nodes, base, s_nodes[base], x, f1, f2, v1, v2, acc);
    walk_tree_grid<kChunk, TWO, kWalk, J + kWalk>(s_nodes, base, x, f1, f2, v1, v2, acc);
  }
}
