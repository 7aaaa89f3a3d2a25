// Deterministic fp64 sums over the rows of a forest kernel (evalcurve.hip, pdp.hip, permimp.hip): per item
// (a tree, a grid point, a job) every wave writes one pair of partial sums (common.h wave_total_f64) to
// part[item][wave][2] and, once, its sum of weights to wpart[wave]; a reduce kernel adds an item's partials
// in a fixed order. Rows beyond a chunk are processed in chunks and the chunk sums added in chunk order, which
// bounds the workspace. No floating-point atomics: the same input gives the same bits on every run.
#pragma once
#include "common.h"
#include <algorithm>

namespace cobalt {

constexpr int kReduceBlock = 256;

// Wave partials of one launch over n rows in blocks of `block`: every wave of every block writes one (the
// last block's waves past the rows write zeros). At most the waves of one row chunk.
inline int64_t wave_parts(int64_t n, int64_t chunk_rows, int block) {
  return (std::min(n, chunk_rows) + block - 1) / block * (block / kWave);
}

// The workspace: [items][parts][2] + [parts] doubles.
inline int64_t wave_partials_bytes(int64_t items, int64_t parts) {
  return (items * parts * 2 + parts) * (int64_t)sizeof(double);
}
inline double* wave_wpart(double* part, int64_t items, int64_t parts) {
  return part ? part + items * parts * 2 : nullptr;
}

// Block k < items: thread i adds the partials i, i + 256, ... (< np; rows of `pitch` pairs) of item k in
// index order, then the 256 thread sums are combined by a fixed LDS tree -> sums[2 k + 0..1]. Block `items`
// does the same for wpart -> sums[2 items] (sum w). `accumulate`: add this row chunk's sums to the earlier
// chunks' (chunk order). k_eval_reduce (evalcurve.hip) is separate: Python reads its [T][3] layout, with
// sum w repeated per tree.
template <int kBlock = kReduceBlock>  // (a template, so that only the files that launch it build it)
static __global__ __launch_bounds__(kBlock) void k_pair_reduce(const double* __restrict__ part,
                                                                     const double* __restrict__ wpart, int pitch,
                                                                     int np, int items, double* __restrict__ sums,
                                                                     int accumulate) {
  __shared__ double s[2][kBlock];
  const int k = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  if (k < items) {
    const double* src = part + (int64_t)k * pitch * 2;
    for (int i = tid; i < np; i += kBlock) {
      a += src[2 * i];
      b += src[2 * i + 1];
    }
  } else {
    for (int i = tid; i < np; i += kBlock) a += wpart[i];
  }
  s[0][tid] = a;
  s[1][tid] = b;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s[0][tid] += s[0][tid + o];
      s[1][tid] += s[1][tid + o];
    }
    __syncthreads();
  }
  if (k < items) {
    if (tid < 2) sums[2 * (int64_t)k + tid] = (accumulate ? sums[2 * (int64_t)k + tid] : 0.0) + s[tid][0];
  } else if (tid == 0) {
    sums[2 * (int64_t)items] = (accumulate ? sums[2 * (int64_t)items] : 0.0) + s[0][0];
  }
}

// A row's metric terms in fp64 from its fp32 margin (widened to m) and label y.
// logloss from the margin: accurate for large |m|.
__device__ __forceinline__ double logloss_term(double m, double y) {
  return log1p(exp(-fabs(m))) + fmax(m, 0.0) - y * m;
}
__device__ __forceinline__ double error_term(float margin, bool ypos) {
  return ((margin > 0.0f) != ypos) ? 1.0 : 0.0;
}

}  // namespace cobalt
