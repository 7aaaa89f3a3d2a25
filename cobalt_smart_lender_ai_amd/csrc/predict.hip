// Tree-ensemble inference (K21) and path-dependent TreeSHAP (K22) for gfx950.
//
// Replaces XGBoost's predictor (`predict_proba`, reference src/api/cobalt_fast_api.py:90-91,
// src/model_train_test/model_tree_train_test.py:171-172) and SHAP's C TreeSHAP extension
// (`shap.TreeExplainer(...).shap_values`, src/api/cobalt_fast_api.py:46,100).
//
// Forest layout (built on the host at model load, ops/predict_ops.py): every tree is renumbered in
// BFS order so the right child is always left+1; a node is 8 bytes
//   uint32 meta = left_child(16 bits, 0xFFFF = leaf) | feature(15 bits) << 16 | default_left << 31
//   float  val  = split threshold (x < val goes left) or leaf value
// Trees are grouped into tiles of <= tile_cap nodes that are staged in LDS; each thread walks
// one row (features staged in LDS with an odd stride, conflict-free) through every tree of the
// tile, accumulating the margin in fp32 in tree order (XGBoost CPU predictor semantics).
//
// TreeSHAP follows the path formulation (every root->leaf path with repeated features merged into
// one element: feature, [lo, hi) interval, NaN-follows flag, product of cover ratios): one thread
// per (row, path) runs EXTEND over the path and the UNWOUND sum per element in fp64, contributions
// are reduced per block in LDS and flushed with one fp64 atomic per (row, feature).
#include "common.h"
#include "forest_walk.h"
#include "knobs.h"
#include "shap_paths.h"
#include <algorithm>

using namespace cobalt;

// ------------------------------------------------------------------------------------ predictor
// ForestBlock (row / tile staging), walk_trees (kWalk trees per thread at once, leaf values delivered in
// tree order) and the tile / LDS limits: forest_walk.h

template <int W>
__global__ __launch_bounds__(256) void k_predict(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                 const uint2* __restrict__ nodes, const int32_t* __restrict__ tree_ptr,
                                                 const int32_t* __restrict__ tile_ptr, int n_tiles, float base_margin,
                                                 float* __restrict__ out_margin, float* __restrict__ out_prob,
                                                 int tile_cap) {
  const ForestBlock<> fb(tile_cap, F, n);
  fb.stage_rows<false>(X, F, ldx);
  float acc = base_margin;
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    if (fb.row < n)
      walk_trees<W>(fb.s_nodes, tree_ptr, nbase, t_begin, t_end, fb.x(), [&](int, float v, uint32_t) { acc += v; });
  }
  if (fb.row < n) {
    if (out_margin) out_margin[fb.row] = acc;
    if (out_prob) out_prob[fb.row] = 1.0f / (1.0f + expf(-acc));
  }
}

COBALT_API int cobalt_predict(const float* X, int64_t n, int F, int64_t ldx, const void* nodes, const int32_t* tree_ptr,
                              const int32_t* tile_ptr, int n_tiles, int tile_cap, float base_margin,
                              float* out_margin, float* out_prob, hipStream_t stream) {
  if (n <= 0) return 0;
  const int block = 256;
  if (const int rc = forest_limits(tile_cap, F, block)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, block);
  static const int walk = [] {
    const int w = cobalt::knob_int(cobalt::Knob::PredWalk, kWalk);
    return (w == 2 || w == 8) ? w : kWalk;
  }();
  const void* fn = walk == 2 ? (const void*)k_predict<2> : walk == 8 ? (const void*)k_predict<8>
                                                                       : (const void*)k_predict<kWalk>;
  static size_t attr_set = kDefaultMaxLds;
  CK(raise_dynamic_lds(fn, lds, attr_set));
  const int grid = ceil_div(n, block);
  const uint2* nd = static_cast<const uint2*>(nodes);
  if (walk == 2)
    hipLaunchKernelGGL(k_predict<2>, dim3(grid), dim3(block), lds, stream, X, n, F, ldx, nd, tree_ptr, tile_ptr,
                       n_tiles, base_margin, out_margin, out_prob, tile_cap);
  else if (walk == 8)
    hipLaunchKernelGGL(k_predict<8>, dim3(grid), dim3(block), lds, stream, X, n, F, ldx, nd, tree_ptr, tile_ptr,
                       n_tiles, base_margin, out_margin, out_prob, tile_cap);
  else
    hipLaunchKernelGGL(k_predict<kWalk>, dim3(grid), dim3(block), lds, stream, X, n, F, ldx, nd, tree_ptr, tile_ptr,
                       n_tiles, base_margin, out_margin, out_prob, tile_cap);
  CK_LAUNCH();
  return 0;
}

// Small/medium batches: the row-block kernel above gives each block ALL trees, so n / 256 blocks
// would leave most CUs idle (a 1-row request streamed the whole 59k-node forest through one CU).
// Here the grid is (row blocks x tree tiles); each block writes its rows' leaf values of its tile's
// trees to leaves[t][row], and k_sum_leaves adds them per row in tree order starting from the base
// margin -- the same fp32 sequence as k_predict, so results are bit-identical across the paths.
__global__ __launch_bounds__(256) void k_predict_leaves(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                        const uint2* __restrict__ nodes,
                                                        const int32_t* __restrict__ tree_ptr,
                                                        const int32_t* __restrict__ tile_ptr,
                                                        float* __restrict__ leaves, int tile_cap) {
  const ForestBlock<> fb(tile_cap, F, n);
  const int tile = blockIdx.y;
  const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
  const int nbase = fb.stage_rows_and_tile(X, F, ldx, nodes, tree_ptr, t_begin, t_end);
  if (fb.row >= n) return;
  walk_trees(fb.s_nodes, tree_ptr, nbase, t_begin, t_end, fb.x(),
             [&](int t, float v, uint32_t) { leaves[(int64_t)t * n + fb.row] = v; });
}

__global__ void k_sum_leaves(const float* __restrict__ leaves, int64_t n, int T, float base_margin,
                             float* __restrict__ out_margin, float* __restrict__ out_prob) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float acc = base_margin;
  for (int t = 0; t < T; ++t) acc += leaves[(int64_t)t * n + row];
  if (out_margin) out_margin[row] = acc;
  if (out_prob) out_prob[row] = 1.0f / (1.0f + expf(-acc));
}

// Rows below which the tile-parallel path is used (fewer than ~2 row blocks per CU otherwise).
COBALT_API int64_t cobalt_predict_small_rows() { return 131072; }

COBALT_API int cobalt_predict_small(const float* X, int64_t n, int F, int64_t ldx, const void* nodes,
                                    const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles, int tile_cap,
                                    int n_trees, float base_margin, float* leaves, float* out_margin,
                                    float* out_prob, hipStream_t stream) {
  if (n <= 0) return 0;
  const int block = 256;
  if (const int rc = forest_limits(tile_cap, F, block)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, block);
  static size_t attr_set = kDefaultMaxLds;
  CK(raise_dynamic_lds((const void*)k_predict_leaves, lds, attr_set));
  hipLaunchKernelGGL(k_predict_leaves, dim3(ceil_div(n, block), n_tiles), dim3(block), lds, stream, X, n, F, ldx,
                     static_cast<const uint2*>(nodes), tree_ptr, tile_ptr, leaves, tile_cap);
  CK_LAUNCH();
  hipLaunchKernelGGL(k_sum_leaves, dim3(ceil_div(n, 256)), dim3(256), 0, stream, leaves, n, n_trees, base_margin,
                     out_margin, out_prob);
  CK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------ TreeSHAP
// PathElem, kShapInv and the canonical summation order (kShapChunk): shap_paths.h
constexpr int kShapMaxF = 80;  // path-parallel kernel: [kShapChunk][F] doubles of LDS

// Path-parallel kernel (small batches): block = (chunk, row), one path per thread; each thread
// writes its path's contributions to its LDS row, then thread f sums column f in path order.
template <int P>
__global__ __launch_bounds__(kShapChunk) void k_treeshap(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                        const PathElem* __restrict__ elems,
                                                        const int32_t* __restrict__ path_ptr,
                                                        const double* __restrict__ path_val, int n_paths, int nchunks,
                                                        double* __restrict__ out) {
  extern __shared__ double s_c[];  // [kShapChunk][F]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.y;
  for (int f = 0; f < F; ++f) s_c[tid * F + f] = 0.0;
  const int p = blockIdx.x * kShapChunk + tid;
  const float* x = X + row * ldx;
  if (p < n_paths) {
    const int e0 = path_ptr[p], k = path_ptr[p + 1] - e0;  // k unique features (bias excluded)
    double z[P], o[P], w[P];
    int feat[P];
    z[0] = 1.0; o[0] = 1.0; w[0] = 1.0; feat[0] = -1;
#pragma unroll
    for (int i = 1; i < P; ++i) { z[i] = 0.0; o[i] = 0.0; w[i] = 0.0; feat[i] = -1; }
    // EXTEND each element
#pragma unroll
    for (int l = 1; l < P; ++l) {
      if (l <= k) {
        const PathElem e = elems[e0 + l - 1];
        const float v = x[e.feat];
        const double one = (v != v) ? (e.nan_ok ? 1.0 : 0.0) : ((v >= e.lo && !(v >= e.hi)) ? 1.0 : 0.0);
        z[l] = e.zero; o[l] = one; feat[l] = e.feat;
        w[l] = 0.0;
#pragma unroll
        for (int j = P - 2; j >= 0; --j) {
          if (j <= l - 1) {
            w[j + 1] += one * w[j] * ((double)(j + 1) / (double)(l + 1));
            w[j] = e.zero * w[j] * ((double)(l - j) / (double)(l + 1));
          }
        }
      }
    }
    const double leaf = path_val[p];
    // UNWOUND sum per element
#pragma unroll
    for (int i = 1; i < P; ++i) {
      if (i <= k) {
        const double one = o[i], zero = z[i];
        double total = 0.0;
        if (one != 0.0) {  // (one is 1 here)
          double next = w[k];
#pragma unroll
          for (int j = P - 2; j >= 0; --j) {
            if (j <= k - 1) {
              const double tmp = next * (1.0 / (double)(j + 1));
              total += tmp;
              next = w[j] - tmp * zero * (double)(k - j);
            }
          }
        } else {
          const double iz = zero != 0.0 ? 1.0 / zero : 0.0;  // zero-cover branch: every w[j] is 0, the term is 0
#pragma unroll
          for (int j = P - 2; j >= 0; --j) {
            if (j <= k - 1) total += w[j] * (iz * kShapInv[k - j]);
          }
        }
        total *= (double)(k + 1);
        s_c[tid * F + feat[i]] = total * (one - zero) * leaf;
      }
    }
  }
  __syncthreads();
  const int np = min(kShapChunk, n_paths - (int)blockIdx.x * kShapChunk);
  for (int f = tid; f < F; f += blockDim.x) {
    double acc = 0.0;
    for (int q = 0; q < np; ++q) acc += s_c[q * F + f];
    out[(row * nchunks + blockIdx.x) * F + f] = acc;
  }
}

// ---------------------------------------------------------------- TreeSHAP with pattern tables
// Fast TreeSHAP "v2" (Yang 2021): the EXTEND/UNWOUND result of a path depends on the row only
// through which of the path's k elements the row satisfies (a k-bit pattern), so all 2^k outcomes
// are tabulated once per model (k_shap_table: the same fp64 arithmetic as k_treeshap, pattern bits
// in place of the row's one-fractions). Scoring a (row, path) is then k interval tests plus k
// table reads. Values and accumulation order equal k_treeshap's, so results are bit-identical.
template <int P>
__global__ void k_shap_table(const PathElem* __restrict__ elems, const int32_t* __restrict__ path_ptr,
                             const double* __restrict__ path_val, int n_paths, const int64_t* __restrict__ tab_ptr,
                             double* __restrict__ table) {
  const int p = blockIdx.x;
  if (p >= n_paths) return;
  const int e0 = path_ptr[p], k = path_ptr[p + 1] - e0;
  const double leaf = path_val[p];
  for (int pat = threadIdx.x; pat < (1 << k); pat += blockDim.x) {
    double z[P], o[P], w[P];
    z[0] = 1.0; o[0] = 1.0; w[0] = 1.0;
#pragma unroll
    for (int i = 1; i < P; ++i) { z[i] = 0.0; o[i] = 0.0; w[i] = 0.0; }
#pragma unroll
    for (int l = 1; l < P; ++l) {
      if (l <= k) {
        const PathElem e = elems[e0 + l - 1];
        const double one = ((pat >> (l - 1)) & 1) ? 1.0 : 0.0;
        z[l] = e.zero; o[l] = one;
        w[l] = 0.0;
#pragma unroll
        for (int j = P - 2; j >= 0; --j) {
          if (j <= l - 1) {
            w[j + 1] += one * w[j] * ((double)(j + 1) / (double)(l + 1));
            w[j] = e.zero * w[j] * ((double)(l - j) / (double)(l + 1));
          }
        }
      }
    }
    double* out = table + tab_ptr[p] + (int64_t)pat * k;
#pragma unroll
    for (int i = 1; i < P; ++i) {
      if (i <= k) {
        const double one = o[i], zero = z[i];
        double total = 0.0;
        if (one != 0.0) {  // (one is 1 here)
          double next = w[k];
#pragma unroll
          for (int j = P - 2; j >= 0; --j) {
            if (j <= k - 1) {
              const double tmp = next * (1.0 / (double)(j + 1));
              total += tmp;
              next = w[j] - tmp * zero * (double)(k - j);
            }
          }
        } else {
          const double iz = zero != 0.0 ? 1.0 / zero : 0.0;  // zero-cover branch: every w[j] is 0, the term is 0
#pragma unroll
          for (int j = P - 2; j >= 0; --j) {
            if (j <= k - 1) total += w[j] * (iz * kShapInv[k - j]);
          }
        }
        total *= (double)(k + 1);
        out[i - 1] = total * (one - zero) * leaf;
      }
    }
  }
}

// Row-parallel kernel (batches): block = (kShapRowsB rows, chunk of paths); every thread walks the
// chunk's paths in order for ITS row: k interval tests -> pattern -> k table values added to its
// private LDS column. A path's elements are the same for every lane, so they come by scalar loads
// (SGPRs) -- no LDS staging of the chunk's elements (which held a block to one per CU: 90 KB of LDS
// for 256 rows, one wave per SIMD) -- and the block is 128 rows: 30 KB of LDS, several blocks per CU.
// Two paths per step: the second path's tests and table loads are issued before the first's adds.
constexpr int kShapRowsF = 48;  // row-parallel kernel: [F][kShapRowsB] doubles of per-row accumulators
constexpr int kShapRowsB = 128;
constexpr int kMaxTabK = 10;

__device__ __forceinline__ int shap_pattern(const PathElem* __restrict__ el, int k, const float* x, int* fe) {
  int pat = 0;
#pragma unroll
  for (int l = 0; l < kMaxTabK; ++l) {
    if (l < k) {
      const PathElem e = el[l];
      const float v = x[e.feat];
      const bool one = (v != v) ? (e.nan_ok != 0) : (v >= e.lo && !(v >= e.hi));
      pat |= (int)one << l;
      fe[l] = e.feat;
    }
  }
  return pat;
}

__global__ __launch_bounds__(kShapRowsB) void k_treeshap_rows(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                              const PathElem* __restrict__ elems,
                                                              const int32_t* __restrict__ path_ptr, int n_paths,
                                                              const int64_t* __restrict__ tab_ptr,
                                                              const double* __restrict__ table, int nchunks,
                                                              double* __restrict__ out) {
  extern __shared__ double s_dyn[];
  constexpr int B = kShapRowsB;
  const int tid = threadIdx.x;
  double* s_phi = s_dyn;                                              // [F][B]
  float* s_x = reinterpret_cast<float*>(s_phi + (size_t)F * B);        // [B][F|1]
  const int xs = F | 1;
  const int c = blockIdx.y;
  const int p0 = c * kShapChunk, p1 = min(n_paths, p0 + kShapChunk);
  const int64_t row0 = (int64_t)blockIdx.x * B;
  const int nrows = (int)min((int64_t)B, n - row0);
  for (int e = tid; e < B * F; e += B) {  // (rows past the batch: zeros, computed and not stored)
    const int r = e / F, f = e - r * F;
    s_x[r * xs + f] = r < nrows ? X[(row0 + r) * ldx + f] : 0.0f;
  }
  for (int f = 0; f < F; ++f) s_phi[f * B + tid] = 0.0;
  __syncthreads();
  const float* x = s_x + tid * xs;
  int p = p0;
  for (; p + 1 < p1; p += 2) {
    const int e0 = path_ptr[p], e1 = path_ptr[p + 1], e2 = path_ptr[p + 2];
    const int ka = e1 - e0, kb = e2 - e1;
    int fa[kMaxTabK], fb[kMaxTabK];
    const int pa = shap_pattern(elems + e0, ka, x, fa);
    const int pb = shap_pattern(elems + e1, kb, x, fb);
    const double* ta = table + tab_ptr[p] + (int64_t)pa * ka;
    const double* tb = table + tab_ptr[p + 1] + (int64_t)pb * kb;
    double va[kMaxTabK], vb[kMaxTabK];
#pragma unroll
    for (int l = 0; l < kMaxTabK; ++l) {
      if (l < ka) va[l] = ta[l];
      if (l < kb) vb[l] = tb[l];
    }
#pragma unroll
    for (int l = 0; l < kMaxTabK; ++l)
      if (l < ka) s_phi[fa[l] * B + tid] += va[l];
#pragma unroll
    for (int l = 0; l < kMaxTabK; ++l)
      if (l < kb) s_phi[fb[l] * B + tid] += vb[l];
  }
  if (p < p1) {
    const int e0 = path_ptr[p], k = path_ptr[p + 1] - e0;
    int fa[kMaxTabK];
    const int pa = shap_pattern(elems + e0, k, x, fa);
    const double* ta = table + tab_ptr[p] + (int64_t)pa * k;
#pragma unroll
    for (int l = 0; l < kMaxTabK; ++l)
      if (l < k) s_phi[fa[l] * B + tid] += ta[l];
  }
  if (tid < nrows) {
    const int64_t row = row0 + tid;
    for (int f = 0; f < F; ++f) out[(row * nchunks + c) * F + f] = s_phi[f * B + tid];
  }
}

__global__ void k_shap_reduce(const double* __restrict__ slab, int64_t n, int F, int nchunks,
                              double* __restrict__ phi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * F) return;
  const int64_t row = i / F;
  const int f = (int)(i - row * F);
  const double* src = slab + row * nchunks * F + f;
  double acc = 0.0;
  for (int c = 0; c < nchunks; ++c) acc += src[(int64_t)c * F];
  phi[i] = acc;
}

// Number of path chunks (and so slab slots per row): fixed by the forest, never by the batch.
COBALT_API int cobalt_treeshap_chunks(int64_t n, int F, int n_paths) {
  (void)n;
  (void)F;
  return n_paths <= 0 ? 1 : (int)ceil_div((int64_t)n_paths, (int64_t)kShapChunk);
}

static int shap_reduce_launch(const double* work, int64_t n, int F, int nchunks, double* phi, hipStream_t stream) {
  const int64_t tot = n * F;
  hipLaunchKernelGGL(k_shap_reduce, dim3((unsigned)ceil_div(tot, (int64_t)256)), dim3(256), 0, stream, work, n, F,
                     nchunks, phi);
  CK_LAUNCH();
  return 0;
}

// Pattern tables exist for paths of <= kMaxTabK unique features (longer: the direct kernel).

COBALT_API int cobalt_shap_table_build(const void* elems, const int32_t* path_ptr, const double* path_val, int n_paths,
                                       int max_len, const int64_t* tab_ptr, double* table, hipStream_t stream) {
  if (n_paths <= 0) return 0;
  if (max_len > kMaxTabK) return -3;
  const PathElem* pe = static_cast<const PathElem*>(elems);
  if (max_len + 1 <= 8)
    hipLaunchKernelGGL(k_shap_table<8>, dim3(n_paths), dim3(128), 0, stream, pe, path_ptr, path_val, n_paths, tab_ptr,
                       table);
  else
    hipLaunchKernelGGL(k_shap_table<kMaxPath>, dim3(n_paths), dim3(256), 0, stream, pe, path_ptr, path_val, n_paths,
                       tab_ptr, table);
  CK_LAUNCH();
  return 0;
}

COBALT_API int cobalt_treeshap_tab(const float* X, int64_t n, int F, int64_t ldx, const void* elems,
                                   const int32_t* path_ptr, int n_paths, int max_len, const int64_t* tab_ptr,
                                   const double* table, double* phi, double* work, int nchunks, hipStream_t stream) {
  if (n <= 0 || n_paths <= 0) return 0;
  if (F > kShapRowsF || max_len > kMaxTabK) return -5;
  if (nchunks != cobalt_treeshap_chunks(n, F, n_paths)) return -8;
  if (nchunks > 1 && work == nullptr) return -7;
  const int B = kShapRowsB;
  const size_t lds = (size_t)F * B * sizeof(double) + (size_t)B * (F | 1) * sizeof(float);
  if (lds > 64 * 1024) CK(hipFuncSetAttribute((const void*)k_treeshap_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_treeshap_rows, dim3((unsigned)ceil_div(n, (int64_t)B), (unsigned)nchunks), dim3(B), lds, stream,
                     X, n, F, ldx, static_cast<const PathElem*>(elems), path_ptr, n_paths, tab_ptr, table, nchunks,
                     nchunks > 1 ? work : phi);
  CK_LAUNCH();
  return nchunks > 1 ? shap_reduce_launch(work, n, F, nchunks, phi, stream) : 0;
}

COBALT_API int cobalt_treeshap(const float* X, int64_t n, int F, int64_t ldx, const void* elems, const int32_t* path_ptr,
                               const double* path_val, int n_paths, int max_len, double* phi, double* work,
                               int nchunks, hipStream_t stream) {
  if (n <= 0 || n_paths <= 0) return 0;
  if (max_len + 1 > kMaxPath) return -3;
  if (n > 65535) return -4;  // grid.y limit; the caller batches rows
  if (F > kShapMaxF) return -5;
  if (nchunks != cobalt_treeshap_chunks(n, F, n_paths)) return -8;
  if (nchunks > 1 && work == nullptr) return -7;
  const size_t lds = (size_t)F * kShapChunk * sizeof(double);
  dim3 grid((unsigned)nchunks, (unsigned)n);
  const PathElem* pe = static_cast<const PathElem*>(elems);
  double* dst = nchunks > 1 ? work : phi;
  if (max_len + 1 <= 8) {
    if (lds > 64 * 1024) CK(hipFuncSetAttribute((const void*)k_treeshap<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_treeshap<8>, grid, dim3(kShapChunk), lds, stream, X, n, F, ldx, pe, path_ptr, path_val,
                       n_paths, nchunks, dst);
  } else {
    if (lds > 64 * 1024) CK(hipFuncSetAttribute((const void*)k_treeshap<kMaxPath>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_treeshap<kMaxPath>, grid, dim3(kShapChunk), lds, stream, X, n, F, ldx, pe, path_ptr, path_val,
                       n_paths, nchunks, dst);
  }
  CK_LAUNCH();
  return nchunks > 1 ? shap_reduce_launch(work, n, F, nchunks, phi, stream) : 0;
}
