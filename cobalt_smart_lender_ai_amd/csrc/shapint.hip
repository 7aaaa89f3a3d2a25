// Path-dependent TreeSHAP interaction values (K22b) for gfx950: `shap.TreeExplainer.shap_interaction_values`
// / XGBoost `pred_interactions` (without the bias row and column), in margin space, covers = sum_hessian.
//
// Works on the merged leaf paths of predict.hip (shap_paths.h). For a path with elements 1..k (zero
// fractions z_e, one fractions o_e in {0, 1}) and leaf value v, the contribution to Phi[i][j], i != j, is
//   1/2 * v * (o_i - z_i) * (o_j - z_j) * W(path \ {i, j})
// where W is the sum of the permutation weights that EXTEND builds over the other k - 2 elements
// (conditioning on j present / absent removes j from the path and scales the leaf by o_j / z_j).
// W is computed by running EXTEND over those k - 2 elements once per unordered pair: products and sums
// of non-negative numbers only -- no UNWIND, so no division by a small zero fraction and no
// cancellation. The diagonal is Phi[i][i] = phi[i] - sum_{j != i} Phi[i][j] with phi the SHAP values
// of predict.hip's kernels.
//
// Layout: one block owns one row and walks the paths in order, R paths at a time:
//   phase 1  thread t computes the pair values of path p0 + t (one (row, path) per thread, fp64) and
//            writes them to its LDS slot, plus a byte map feature -> position in the path;
//   phase 2  thread c owns the unordered feature pairs c, c + R, ...; it walks the R paths in order and
//            adds the values of the paths that hold both features to the pair's accumulator.
// Summation order (canonical, shap_paths.h): path order within a chunk of kShapChunk paths, then the
// chunk sums in chunk order. Nothing depends on the batch or on the block size R, so a row's values are
// bit-identical for any batch size, position in the batch and kernel variant. No floating-point
// atomics. Each unordered pair is computed once and stored to both cells: the output is exactly
// symmetric.
//
// Memory bound: the kernel uses no global scratch at all -- the F (F - 1) / 2 accumulators of a row
// live in LDS (cobalt_treeshap_interactions_lds bytes per block: 51 KB at F = 20, 74 KB at F = 48 for
// paths of <= 7 features), whatever N is. The caller supplies phi [n, F].
#include "common.h"
#include "shap_paths.h"

using namespace cobalt;

namespace {
constexpr int kShapIntMaxF = 48;  // 1128 pair accumulators x 2 + a [R][F] byte map next to the pair values

__host__ __device__ constexpr int shapint_pairs(int P) { return (P - 1) * (P - 2) / 2; }

// One EXTEND step of element (zero, one) on a path that holds l - 1 elements (and the bias) so far;
// the operation order of predict.hip's kernels.
#define SHAPINT_EXTEND_STEP(w, j, l, one, zero)                                     \
  do {                                                                              \
    (w)[(j) + 1] += (one) * (w)[(j)] * ((double)((j) + 1) / (double)((l) + 1));     \
    (w)[(j)] = (zero) * (w)[(j)] * ((double)((l) - (j)) / (double)((l) + 1));       \
  } while (0)

// Pair values of one path, every loop unrolled (the ratios fold to constants, arrays stay in VGPRs).
template <int P>
__device__ __forceinline__ void pair_values_unrolled(const double (&z)[P], const double (&o)[P], int k, double leaf,
                                                     double* __restrict__ val) {
#pragma unroll
  for (int a = 1; a < P; ++a) {
#pragma unroll
    for (int b = a + 1; b < P; ++b) {
      if (b <= k) {
        double w[P - 1];
        w[0] = 1.0;
#pragma unroll
        for (int j = 1; j < P - 1; ++j) w[j] = 0.0;
#pragma unroll
        for (int e = 1; e < P; ++e) {
          if (e != a && e != b && e <= k) {
            const int l = e - (e > a ? 1 : 0) - (e > b ? 1 : 0);
#pragma unroll
            for (int j = P - 3; j >= 0; --j)
              if (j <= l - 1) SHAPINT_EXTEND_STEP(w, j, l, o[e], z[e]);
          }
        }
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < P - 2; ++j) sum += w[j];  // (entries past k - 2 are zero)
        const double s = (o[a] - z[a]) * (o[b] - z[b]);
        val[(b - 1) * (b - 2) / 2 + (a - 1)] = 0.5 * leaf * s * sum;
      }
    }
  }
}

// The same arithmetic with run-time loops (paths of up to kMaxPath - 1 features: 105 pairs, unrolling
// them would be ~20k EXTEND steps of code).
template <int P>
__device__ void pair_values_loop(const double (&z)[P], const double (&o)[P], int k, double leaf,
                                 double* __restrict__ val) {
  for (int a = 1; a <= k; ++a) {
    for (int b = a + 1; b <= k; ++b) {
      double w[P - 1];
      w[0] = 1.0;
      for (int j = 1; j < P - 1; ++j) w[j] = 0.0;
      int l = 0;
      for (int e = 1; e <= k; ++e) {
        if (e == a || e == b) continue;
        ++l;
        for (int j = l - 1; j >= 0; --j) SHAPINT_EXTEND_STEP(w, j, l, o[e], z[e]);
      }
      double sum = 0.0;
      for (int j = 0; j <= k - 2; ++j) sum += w[j];
      const double s = (o[a] - z[a]) * (o[b] - z[b]);
      val[(b - 1) * (b - 2) / 2 + (a - 1)] = 0.5 * leaf * s * sum;
    }
  }
}

__host__ __device__ inline int shapint_pos_stride(int F) { return (F + 3) & ~3; }
__host__ __device__ inline int shapint_cells(int F) { return F * (F - 1) / 2; }

// Dynamic LDS of a block: pair values [R][NP], chunk and total accumulators [cells] each, the
// diagonal [F], the row [F] and the position map [R][F rounded up to 4] bytes.
inline size_t shapint_lds(int F, int R, int NP) {
  return (size_t)R * NP * sizeof(double) + (size_t)(2 * shapint_cells(F) + F) * sizeof(double) +
         (size_t)shapint_pos_stride(F) * sizeof(float) + (size_t)R * shapint_pos_stride(F);
}

// P - 1 = longest path (unique features) the variant takes, R = block size = paths per step (divides
// kShapChunk).
template <int P, int R, bool kUnrolled>
__global__ __launch_bounds__(R) void k_shap_interactions(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                        const PathElem* __restrict__ elems,
                                                        const int32_t* __restrict__ path_ptr,
                                                        const double* __restrict__ path_val, int n_paths,
                                                        const double* __restrict__ phi, double* __restrict__ out) {
  static_assert(kShapChunk % R == 0, "a chunk is a whole number of steps");
  constexpr int NP = shapint_pairs(P);
  extern __shared__ double s_dyn[];
  const int tid = threadIdx.x;
  const int cells = shapint_cells(F);
  const int fs = shapint_pos_stride(F);
  double* s_val = s_dyn;                                   // [R][NP]
  double* s_chunk = s_val + (size_t)R * NP;                 // [cells] sum of the current chunk
  double* s_tot = s_chunk + cells;                          // [cells] sum of the finished chunks
  double* s_diag = s_tot + cells;                           // [F]
  float* s_x = reinterpret_cast<float*>(s_diag + F);        // [fs]
  uint8_t* s_pos = reinterpret_cast<uint8_t*>(s_x + fs);    // [R][fs] position of a feature in the path
  const int64_t row = blockIdx.x;
  if (row >= n) return;
  for (int c = tid; c < cells; c += R) { s_chunk[c] = 0.0; s_tot[c] = 0.0; }
  for (int f = tid; f < F; f += R) s_x[f] = X[row * ldx + f];
  __syncthreads();

  for (int p0 = 0; p0 < n_paths; p0 += R) {
    // ---- phase 1: this thread's path
    uint32_t* my_pos = reinterpret_cast<uint32_t*>(s_pos + (size_t)tid * fs);
    for (int i = 0; i < fs / 4; ++i) my_pos[i] = 0xFFFFFFFFu;
    const int p = p0 + tid;
    if (p < n_paths) {
      const int e0 = path_ptr[p];
      const int k = min(path_ptr[p + 1] - e0, P - 1);  // (the host refuses longer paths)
      double z[P], o[P];
      z[0] = 1.0; o[0] = 1.0;
#pragma unroll
      for (int l = 1; l < P; ++l) {
        z[l] = 0.0; o[l] = 0.0;
        if (l <= k) {
          const PathElem e = elems[e0 + l - 1];
          if ((unsigned)e.feat < (unsigned)F) {
            const float v = s_x[e.feat];
            o[l] = (v != v) ? (e.nan_ok ? 1.0 : 0.0) : ((v >= e.lo && !(v >= e.hi)) ? 1.0 : 0.0);
            s_pos[(size_t)tid * fs + e.feat] = (uint8_t)(l - 1);
          }
          z[l] = e.zero;
        }
      }
      if (k >= 2) {
        const double leaf = path_val[p];
        if (kUnrolled) pair_values_unrolled<P>(z, o, k, leaf, s_val + (size_t)tid * NP);
        else pair_values_loop<P>(z, o, k, leaf, s_val + (size_t)tid * NP);
      }
    }
    __syncthreads();
    // ---- phase 2: this thread's feature pairs, the step's paths in order
    const int np = min(R, n_paths - p0);
    const bool chunk_end = ((p0 + R) % kShapChunk == 0) || (p0 + R >= n_paths);
    for (int c = tid; c < cells; c += R) {
      // cell c = j (j - 1) / 2 + i, i < j
      int j = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)c)) * 0.5f);
      while (j * (j - 1) / 2 > c) --j;
      while ((j + 1) * j / 2 <= c) ++j;
      const int i = c - j * (j - 1) / 2;
      double acc = s_chunk[c];
      for (int t = 0; t < np; ++t) {
        const int pa = s_pos[t * fs + i], pb = s_pos[t * fs + j];
        if (pa != 0xFF && pb != 0xFF) {
          const int lo = min(pa, pb), hi = max(pa, pb);
          acc += s_val[t * NP + hi * (hi - 1) / 2 + lo];
        }
      }
      if (chunk_end) {
        s_tot[c] += acc;
        acc = 0.0;
      }
      s_chunk[c] = acc;
    }
    __syncthreads();
  }

  // ---- diagonal from phi and the off-diagonals (ascending j), then the whole matrix in one sweep
  for (int f = tid; f < F; f += R) {
    double s = 0.0;
    for (int j = 0; j < F; ++j) {
      if (j == f) continue;
      const int lo = min(f, j), hi = max(f, j);
      s += s_tot[hi * (hi - 1) / 2 + lo];
    }
    s_diag[f] = phi[row * F + f] - s;
  }
  __syncthreads();
  double* dst = out + row * (int64_t)F * F;
  for (int e = tid; e < F * F; e += R) {
    const int i = e / F, j = e - i * F;
    const int lo = min(i, j), hi = max(i, j);
    dst[e] = (i == j) ? s_diag[i] : s_tot[hi * (hi - 1) / 2 + lo];
  }
}

template <int P, int R, bool kUnrolled>
int shapint_launch(const float* X, int64_t n, int F, int64_t ldx, const PathElem* elems, const int32_t* path_ptr,
                   const double* path_val, int n_paths, const double* phi, double* out, hipStream_t stream) {
  const size_t lds = shapint_lds(F, R, shapint_pairs(P));
  if (lds > 160 * 1024) return -5;
  static size_t attr_set = 64 * 1024;
  if (lds > attr_set) {
    CK(hipFuncSetAttribute((const void*)k_shap_interactions<P, R, kUnrolled>,
                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = lds;
  }
  hipLaunchKernelGGL((k_shap_interactions<P, R, kUnrolled>), dim3((unsigned)n), dim3(R), lds, stream, X, n, F, ldx,
                     elems, path_ptr, path_val, n_paths, phi, out);
  CK_LAUNCH();
  return 0;
}
}  // namespace

// Widest model the interaction kernel takes.
COBALT_API int cobalt_treeshap_interactions_max_f() { return kShapIntMaxF; }

// LDS bytes per block for a model of F features and paths of up to max_len features (-1: outside the limits).
COBALT_API int64_t cobalt_treeshap_interactions_lds(int F, int max_len) {
  if (F < 1 || F > kShapIntMaxF || max_len + 1 > kMaxPath) return -1;
  return max_len + 1 <= 8 ? (int64_t)shapint_lds(F, 256, shapint_pairs(8))
                          : (int64_t)shapint_lds(F, 64, shapint_pairs(kMaxPath));
}

// out [n, F, F] float64 from X [n, F] (row stride ldx) and phi [n, F] (the rows' SHAP values).
// -3: a path longer than kMaxPath - 1 features; -4: too many rows for one launch; -5: F outside
// 1..kShapIntMaxF; -6: a null buffer. Nothing is launched on an error.
COBALT_API int cobalt_treeshap_interactions(const float* X, int64_t n, int F, int64_t ldx, const void* elems,
                                            const int32_t* path_ptr, const double* path_val, int n_paths, int max_len,
                                            const double* phi, double* out, hipStream_t stream) {
  if (n <= 0) return 0;
  if (F < 1 || F > kShapIntMaxF) return -5;
  if (max_len + 1 > kMaxPath) return -3;
  if (n > 0x7FFFFFFF) return -4;
  if (n_paths < 0 || ldx < F) return -6;
  // (a forest of single-leaf trees has paths and no element: max_len 0, elems is never read)
  if (!X || !phi || !out || (n_paths > 0 && (!path_ptr || !path_val)) || (max_len > 0 && !elems)) return -6;
  const PathElem* pe = static_cast<const PathElem*>(elems);
  if (max_len + 1 <= 8)
    return shapint_launch<8, 256, true>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, phi, out, stream);
  return shapint_launch<kMaxPath, 64, false>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, phi, out, stream);
}
