// Leaf-path representation and constants shared by the TreeSHAP kernels (predict.hip: SHAP values,
// shapint.hip: SHAP interaction values). The host packs the paths in ops/predict_ops.py
// (extract_paths, PATH_ELEM).
#pragma once
#include "common.h"

struct PathElem {
  float lo, hi;        // row follows the path on this feature iff x >= lo && !(x >= hi) (non-missing);
                       // no upper bound: hi = NaN (+inf would turn x = +inf away), no lower bound: lo = -inf
  int32_t feat;        // feature index
  int32_t nan_ok;      // row with NaN follows the path on this feature
  double zero;         // product of cover(child)/cover(parent) over the merged occurrences
};
static_assert(sizeof(PathElem) == 24, "PathElem");

constexpr int kMaxPath = 16;       // max unique elements per path (incl. bias) in the SHAP kernels

// EXTEND / UNWIND without per-step divisions: the integer ratios (j + 1) / (l + 1) fold to constants of
// the unrolled loops, 1 / (k - j) comes from kShapInv and 1 / zero is taken once per element; both SHAP
// kernels (and so the pattern tables) use the same operation order, so their values stay bit-identical
// to each other (and within rounding of the division form and of the host oracle).
static __constant__ double kShapInv[18] = {0.0,       1.0,        1.0 / 2,  1.0 / 3,  1.0 / 4,  1.0 / 5,
                                           1.0 / 6,   1.0 / 7,    1.0 / 8,  1.0 / 9,  1.0 / 10, 1.0 / 11,
                                           1.0 / 12,  1.0 / 13,   1.0 / 14, 1.0 / 15, 1.0 / 16, 1.0 / 17};

// Canonical summation order (shared by every SHAP kernel, so a row's values do not depend on the
// batch size or on which kernel ran): paths are cut into fixed chunks of kShapChunk; within a chunk
// contributions are added in path order; the chunk sums are added in chunk order. No floating-point
// atomics anywhere.
constexpr int kShapChunk = 256;
