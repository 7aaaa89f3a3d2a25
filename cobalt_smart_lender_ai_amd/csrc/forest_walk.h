// The packed-forest walk shared by the predictor (predict.hip) and the learning-curve pass
// (evalcurve.hip). Forest layout (ops/predict_ops.py pack_forest): BFS-numbered trees, 8-byte nodes
//   uint32 meta = left_child(16 bits, 0xFFFF = leaf) | feature(15 bits) << 16 | default_left << 31
//   float  val  = split threshold (x < val goes left) or leaf value
// grouped into tiles that the caller stages in LDS.
#pragma once
#include "common.h"

// A tree walk is a chain of dependent LDS reads (node -> feature value -> next node), so one
// thread walks kWalk trees at once: the kWalk chains' loads are independent and overlap. The leaf
// values are still added to the margin one tree at a time in tree order (same fp32 sum).
// kWalk is the default; COBALT_PRED_WALK=2|8 selects the other instantiations for sweeps.
constexpr int kWalk = 4;

template <int kWalk = ::kWalk, typename Leaf>
__device__ __forceinline__ void walk_trees(const uint2* s_nodes, const int32_t* __restrict__ tree_ptr, int nbase,
                                           int t_begin, int t_end, const float* x, Leaf&& leaf) {
  for (int t = t_begin; t < t_end; t += kWalk) {
    uint32_t base[kWalk];
    uint2 nd[kWalk];
#pragma unroll
    for (int k = 0; k < kWalk; ++k) {  // past the tile's end: walk tree t again, result unused
      base[k] = (uint32_t)(tree_ptr[t + k < t_end ? t + k : t] - nbase);
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
          nd[k] = s_nodes[base[k] + (nd[k].x & 0xFFFFu) + (left ? 0u : 1u)];
          more = true;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kWalk; ++k)
      if (t + k < t_end) leaf(t + k, __uint_as_float(nd[k].y));
  }
}
