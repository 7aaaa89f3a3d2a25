// Learning curve of a tree ensemble on a labelled row set in ONE pass over the forest (gfx950).
//
// XGBoost reports the validation metric after every boosting round (`evals=`, `eval_set=`) and
// early stopping reads that curve. Scoring every prefix with the predictor would walk 1 + 2 + ... + T
// trees; here each row walks the forest once, in tree order, and the metric terms are emitted after
// every tree.
//
// A client of the packed-forest block of forest_walk.h (ForestBlock, walk_trees), like the predictor: one
// thread owns one row (features staged in LDS with an odd stride), tiles of the forest are staged in
// LDS, and the margin is accumulated in fp32 in tree order -- the margin after tree t has the bits of
// `predict_margin(n_trees = t + 1)`. After each tree the row's terms are computed in fp64 from that
// fp32 margin m:
//   logloss  log1p(exp(-|m|)) + max(m, 0) - y m     (wave_partials.h logloss_term)
//   error    (m > 0) != (y > 0.5)                   (error_term)
// and reduced deterministically (wave_partials.h; no floating-point atomics): the 64 lanes of a wave are
// summed by a fixed DPP sequence, the wave's pair goes to workspace[tree][wave], and k_eval_reduce adds a tree's
// partials in a fixed order. Rows beyond kEvalChunkRows are processed in chunks of that many rows
// (which bounds the workspace); chunk sums are added in chunk order. The same input gives the same
// bits on every run.
#include "common.h"
#include "forest_walk.h"
#include "wave_partials.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kEvalBlock = 256;
constexpr int64_t kEvalChunkRows = 1 << 19;  // rows per launch (whole blocks): 8192 wave partials per tree
}  // namespace

// Rows [0, n) of one chunk; `stage` (nullable) points at the chunk's first row of the [n_trees, stage_ld]
// matrix. METRICS: y / part / wpart are set and every wave writes part[tree][wave] = (sum w loss,
// sum w err) and wpart[wave] = sum w. Rows past n (the last block) walk a row of zeros with weight 0, so
// that every lane takes part in the wave sums.
template <bool METRICS>
__global__ __launch_bounds__(kEvalBlock) void k_eval_curve(
    const float* __restrict__ X, int64_t n, int F, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ w, const uint2* __restrict__ nodes, const int32_t* __restrict__ tree_ptr,
    const int32_t* __restrict__ tile_ptr, int n_tiles, float base_margin, const float* __restrict__ margin_in,
    float* __restrict__ margin_out, float* __restrict__ stage, int64_t stage_ld, double* __restrict__ part,
    double* __restrict__ wpart, int nparts, int tile_cap) {
  const ForestBlock<kEvalBlock> fb(tile_cap, F, n);
  const int64_t row = fb.row;
  const bool valid = row < n;
  fb.stage_rows<true>(X, F, ldx);
  float acc = (valid && margin_in) ? margin_in[row] : base_margin;
  double yv = 0.0, wv = 0.0;
  bool ypos = false;
  const int wave_g = blockIdx.x * (kEvalBlock / kWave) + wave_id();  // < nparts
  if constexpr (METRICS) {
    if (valid) {
      const float yf = y[row];
      yv = (double)yf;
      ypos = yf > 0.5f;
      wv = w ? (double)w[row] : 1.0;
    }
    const double sw = wave_total_f64(wv);
    if (lane_id() == kWave - 1) wpart[wave_g] = sw;
  }
  const float* x = fb.x();
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    walk_trees(fb.s_nodes, tree_ptr, nbase, t_begin, t_end, x, [&](int t, float v, uint32_t) {
      acc += v;
      if (stage && valid) stage[(int64_t)t * stage_ld + row] = acc;
      if constexpr (METRICS) {
        const double m = (double)acc;
        const double loss = logloss_term(m, yv);
        const double err = error_term(acc, ypos);
        const double sl = wave_total_f64(wv * loss);
        const double se = wave_total_f64(wv * err);
        if (lane_id() == kWave - 1) {
          double* dst = part + ((int64_t)t * nparts + wave_g) * 2;
          dst[0] = sl;
          dst[1] = se;
        }
      }
    });
  }
  if (valid && margin_out) margin_out[row] = acc;
}

// One block per tree: thread i adds partials i, i + 256, ... (< nparts, the chunk's waves; rows of `pitch`
// pairs) in index order, then the 256 thread sums are combined by a fixed LDS tree. `accumulate`: add this
// chunk's sums to the earlier chunks' (chunk order).
__global__ __launch_bounds__(kReduceBlock) void k_eval_reduce(const double* __restrict__ part,
                                                              const double* __restrict__ wpart, int pitch,
                                                              int nparts, double* __restrict__ sums,
                                                              int accumulate) {
  __shared__ double s[3][kReduceBlock];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* src = part + (int64_t)t * pitch * 2;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = tid; i < nparts; i += kReduceBlock) {
    a += src[2 * i];
    b += src[2 * i + 1];
    c += wpart[i];
  }
  s[0][tid] = a;
  s[1][tid] = b;
  s[2][tid] = c;
  __syncthreads();
  for (int o = kReduceBlock / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s[0][tid] += s[0][tid + o];
      s[1][tid] += s[1][tid + o];
      s[2][tid] += s[2][tid + o];
    }
    __syncthreads();
  }
  if (tid < 3) sums[t * 3 + tid] = (accumulate ? sums[t * 3 + tid] : 0.0) + s[tid][0];
}

static int64_t eval_parts(int64_t n) { return wave_parts(n, kEvalChunkRows, kEvalBlock); }

// Bytes of `workspace` for n rows and n_trees trees: [n_trees][parts][2] + [parts] doubles with
// parts = the waves of one row chunk.
COBALT_API int64_t cobalt_eval_curve_workspace(int64_t n, int n_trees) {
  if (n <= 0 || n_trees <= 0) return 0;
  return wave_partials_bytes(n_trees, eval_parts(n));
}

// y == nullptr: no metrics (margins / stage margins only; w, workspace and sums are not touched).
// Returns -2 / -3 for a tile or an LDS footprint outside the limits (as cobalt_predict), -7 when metrics
// are asked for without workspace or sums; nothing is launched then.
COBALT_API int cobalt_eval_curve(const float* X, int64_t n, int F, int64_t ldx, const float* y, const float* w,
                                 const void* nodes, const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles,
                                 int tile_cap, int n_trees, float base_margin, const float* margin_in,
                                 float* margin_out, float* stage_margins, void* workspace, double* sums,
                                 hipStream_t stream) {
  if (n <= 0 || n_trees <= 0) return 0;
  if (const int rc = forest_limits(tile_cap, F, kEvalBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kEvalBlock);
  const bool metrics = y != nullptr;
  if (metrics && (workspace == nullptr || sums == nullptr)) return -7;
  const void* fn = metrics ? (const void*)k_eval_curve<true> : (const void*)k_eval_curve<false>;
  static size_t attr_set[2] = {kDefaultMaxLds, kDefaultMaxLds};
  CK(raise_dynamic_lds(fn, lds, attr_set[metrics]));
  const uint2* nd = static_cast<const uint2*>(nodes);
  const int nparts = (int)eval_parts(n);
  double* part = static_cast<double*>(workspace);
  double* wpart = wave_wpart(part, n_trees, nparts);
  for (int64_t r0 = 0; r0 < n; r0 += kEvalChunkRows) {
    const int64_t nc = std::min(kEvalChunkRows, n - r0);
    const int grid = ceil_div(nc, kEvalBlock);
    const int np = (int)eval_parts(nc);  // <= nparts; the partials keep the pitch nparts
    const float* mi = margin_in ? margin_in + r0 : nullptr;
    float* mo = margin_out ? margin_out + r0 : nullptr;
    float* st = stage_margins ? stage_margins + r0 : nullptr;
    if (metrics) {
      hipLaunchKernelGGL(k_eval_curve<true>, dim3(grid), dim3(kEvalBlock), lds, stream, X + r0 * ldx, nc, F, ldx,
                         y + r0, w ? w + r0 : nullptr, nd, tree_ptr, tile_ptr, n_tiles, base_margin, mi, mo, st, n,
                         part, wpart, nparts, tile_cap);
      CK_LAUNCH();
      hipLaunchKernelGGL(k_eval_reduce, dim3(n_trees), dim3(kReduceBlock), 0, stream, part, wpart, nparts, np, sums,
                         r0 > 0 ? 1 : 0);
      CK_LAUNCH();
    } else {
      hipLaunchKernelGGL(k_eval_curve<false>, dim3(grid), dim3(kEvalBlock), lds, stream, X + r0 * ldx, nc, F, ldx,
                         nullptr, nullptr, nd, tree_ptr, tile_ptr, n_tiles, base_margin, mi, mo, st, n, nullptr,
                         nullptr, nparts, tile_cap);
      CK_LAUNCH();
    }
  }
  return 0;
}
