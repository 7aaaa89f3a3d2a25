// Interventional TreeSHAP against a background set (K22c) for gfx950: `shap.TreeExplainer(model, data,
// feature_perturbation="interventional")`, in margin space or with shap's per-pair rescaling to
// probability space (`model_output="probability"`). Node covers are not used.
//
// For an explained row x and a background row z the game is v(S) = f(x on S, z elsewhere). On a merged
// leaf path (shap_paths.h) with leaf value v every unique feature is satisfied by x, by z, by both or
// by neither. A feature satisfied by neither row kills the path. Otherwise, with a features only x
// satisfies and b only z satisfies (a + b > 0),
//   each x-only feature gets  + v (a - 1)! b! / (a + b)!
//   each z-only feature gets  - v a! (b - 1)! / (a + b)!
// and phi(x) = 1/B sum_z s(x, z) phi(x, z), s = 1 (margin) or
// s = (sigmoid f(x) - sigmoid f(z)) / (f(x) - f(z)) (probability), f = the float64 sum of the base
// margin and the leaf values in tree order.
//
// Two kernels per background tile (the host tiles over the rows of X and over the background):
//   k_shapbg_masks  one block per row, one thread per path: the 16-bit mask of the path elements the
//                   row satisfies, [rows, n_paths], and the row's float64 margin (the leaves of the
//                   satisfied paths, added in path order by one thread). Run on the background tile;
//                   in probability mode also on the rows of X (margins only).
//   k_shapbg        one block per explained row, one thread per path, 256 paths a step. A thread takes
//                   its x-mask once and walks the background tile: two AND, two popcounts, two weight
//                   table reads and one predicated float64 add per path element into accumulators
//                   that stay in registers. The element sums of a step are then reduced by feature.
// Summation order (fixed, independent of the batch): a path element sums its background rows in
// order within a tile; a feature sums groups of 64 consecutive paths in path order and adds the group
// sums in group order; tiles are added in tile order (the first tile stores, later tiles add to phi)
// and the last tile divides by B. No floating-point atomics: a row's values are bit-identical across
// runs, batch sizes and positions in the batch.
//
// Workspace (caller's): masks [tile, n_paths] uint16 and margins [tile] float64 of a background tile,
// margins [rows] of an X tile in probability mode; nothing grows with N or B.
#include "common.h"
#include "shap_paths.h"

using namespace cobalt;

namespace {
constexpr int kBgBlock = 256;      // threads per block = paths per step (= kShapChunk)
constexpr int kBgGroup = 64;       // paths per ordered group sum
constexpr int kBgGroups = kBgBlock / kBgGroup;
constexpr int kBgMaxF = 256;       // widest X: the [256][F] byte map of a step stays within 64 KB
constexpr int kBgMaxTile = 1024;   // background rows per launch (their rescaling factors sit in LDS)
static_assert(kBgBlock == kShapChunk, "a step is a chunk");

constexpr double bg_fact(int n) { return n <= 1 ? 1.0 : (double)n * bg_fact(n - 1); }

// W[a][b] = (a - 1)! b! / (a + b)! for a >= 1, a + b <= kMaxPath - 1 (integers below 2^53 divided once:
// correctly rounded); 0 elsewhere, so a = 0 needs no branch. The z-only weight is W[b][a].
struct BgWeights {
  double w[kMaxPath * kMaxPath];
  constexpr BgWeights() : w() {
    for (int a = 0; a < kMaxPath; ++a)
      for (int b = 0; b < kMaxPath; ++b)
        w[a * kMaxPath + b] = (a >= 1 && a + b <= kMaxPath - 1) ? bg_fact(a - 1) * bg_fact(b) / bg_fact(a + b) : 0.0;
  }
};
__device__ const BgWeights kBgWeights{};

__device__ __forceinline__ bool bg_follows(const PathElem& e, float v) {
  return (v != v) ? (e.nan_ok != 0) : (v >= e.lo && !(v >= e.hi));
}

// Mask of the elements of path p the row in s_x satisfies (bit l = element l; bits from k up are 0).
__device__ __forceinline__ unsigned bg_mask(const float* s_x, int F, const PathElem* __restrict__ elems, int e0, int k) {
  unsigned m = 0;
  for (int l = 0; l < k; ++l) {
    const PathElem e = elems[e0 + l];
    if ((unsigned)e.feat < (unsigned)F && bg_follows(e, s_x[e.feat])) m |= 1u << l;
  }
  return m;
}

// (sigmoid(a) - sigmoid(b)) / (a - b) without the cancellation of that quotient:
// sigmoid(hi) sigmoid(-lo) (1 - exp(-d)) / d with d = hi - lo >= 0; d = 0 gives the derivative.
__device__ __forceinline__ double bg_rescale(double a, double b) {
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  const double d = hi - lo;
  const double r = d == 0.0 ? 1.0 : -expm1(-d) / d;
  return (1.0 / (1.0 + exp(-hi))) * (1.0 / (1.0 + exp(lo))) * r;
}

__global__ __launch_bounds__(kBgBlock) void k_shapbg_masks(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                          const PathElem* __restrict__ elems,
                                                          const int32_t* __restrict__ path_ptr,
                                                          const double* __restrict__ path_val, int n_paths,
                                                          double base_margin, uint16_t* __restrict__ masks,
                                                          double* __restrict__ margins) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_leaf[kBgBlock];
  __shared__ unsigned long long s_full[kBgBlock / kWave];
  float* s_x = reinterpret_cast<float*>(s_raw);  // [F]
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  if (row >= n) return;
  for (int f = tid; f < F; f += kBgBlock) s_x[f] = X[row * ldx + f];
  __syncthreads();
  double margin = base_margin;  // (thread 0's copy is the one that counts)
  for (int p0 = 0; p0 < n_paths; p0 += kBgBlock) {
    const int p = p0 + tid;
    bool full = false;
    if (p < n_paths) {
      const int e0 = path_ptr[p];
      const int k = min(path_ptr[p + 1] - e0, kMaxPath - 1);  // (the host refuses longer paths)
      const unsigned m = bg_mask(s_x, F, elems, e0, k);
      if (masks) masks[row * (int64_t)n_paths + p] = (uint16_t)m;
      full = m == (1u << k) - 1u;
      if (full) s_leaf[tid] = path_val[p];
    }
    const unsigned long long bal = __ballot(full);
    if (lane_id() == 0) s_full[wave_id()] = bal;
    __syncthreads();
    if (tid == 0) {
      for (int w = 0; w < kBgBlock / kWave; ++w) {
        unsigned long long m = s_full[w];
        while (m) {
          margin += s_leaf[w * kWave + __builtin_ctzll(m)];
          m &= m - 1;
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) margins[row] = margin;
}

__host__ __device__ inline int bg_pos_stride(int F) { return (F + 15) & ~15; }

// Dynamic LDS of k_shapbg: element sums [256][P - 1], group sums [4][F], totals [F], rescaling factors
// [tile] (probability mode), the row [F rounded up] and the feature -> element map [256][F rounded up]
// bytes. Every region starts on a multiple of 16 bytes.
inline size_t bg_lds(int F, int P, int tile) {
  const int fs = bg_pos_stride(F);
  return (size_t)kBgBlock * (P - 1) * sizeof(double) + (size_t)(kBgGroups + 1) * fs * sizeof(double) +
         (size_t)((tile + 1) & ~1) * sizeof(double) + (size_t)fs * sizeof(float) + (size_t)kBgBlock * fs;
}

// P - 1 = longest path (unique features) the variant takes.
template <int P, bool kProb>
__global__ __launch_bounds__(kBgBlock) void k_shapbg(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                    const PathElem* __restrict__ elems,
                                                    const int32_t* __restrict__ path_ptr,
                                                    const double* __restrict__ path_val, int n_paths,
                                                    const uint16_t* __restrict__ zmask,
                                                    const double* __restrict__ zmargin, int nb,
                                                    const double* __restrict__ xmargin, int first, int last,
                                                    double n_background, double* __restrict__ phi) {
  constexpr int E = P - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  __shared__ double s_w[kMaxPath * kMaxPath];
  const int tid = threadIdx.x;
  const int fs = bg_pos_stride(F);
  double* s_val = reinterpret_cast<double*>(s_raw);          // [256][E]
  double* s_part = s_val + (size_t)kBgBlock * E;             // [4][fs] group sums of the step
  double* s_tot = s_part + (size_t)kBgGroups * fs;           // [fs]
  double* s_s = s_tot + fs;                                  // [tile rounded up to 2]
  float* s_x = reinterpret_cast<float*>(s_s + (kProb ? ((nb + 1) & ~1) : 0));  // [fs]
  uint8_t* s_pos = reinterpret_cast<uint8_t*>(s_x + fs);     // [256][fs] element of a feature in the path
  const int64_t row = blockIdx.x;
  if (row >= n) return;
  for (int i = tid; i < kMaxPath * kMaxPath; i += kBgBlock) s_w[i] = kBgWeights.w[i];
  for (int f = tid; f < F; f += kBgBlock) {
    s_x[f] = X[row * ldx + f];
    s_tot[f] = 0.0;
  }
  if (kProb) {
    const double fx = xmargin[row];
    for (int b = tid; b < nb; b += kBgBlock) s_s[b] = bg_rescale(fx, zmargin[b]);
  }
  __syncthreads();

  for (int p0 = 0; p0 < n_paths; p0 += kBgBlock) {
    // ---- phase 1: this thread's path against every background row of the tile
    uint32_t* my_pos = reinterpret_cast<uint32_t*>(s_pos + (size_t)tid * fs);
    for (int i = 0; i < fs / 4; ++i) my_pos[i] = 0xFFFFFFFFu;
    const int p = p0 + tid;
    if (p < n_paths) {
      const int e0 = path_ptr[p];
      const int k = min(path_ptr[p + 1] - e0, E);  // (the host refuses longer paths)
      unsigned xm = 0;
      for (int l = 0; l < k; ++l) {
        const PathElem e = elems[e0 + l];
        if ((unsigned)e.feat < (unsigned)F) {
          if (bg_follows(e, s_x[e.feat])) xm |= 1u << l;
          s_pos[(size_t)tid * fs + e.feat] = (uint8_t)l;
        }
      }
      const unsigned full = (1u << k) - 1u;
      double acc[E];
#pragma unroll
      for (int l = 0; l < E; ++l) acc[l] = 0.0;
      const uint16_t* zp = zmask + p;
#pragma unroll 4
      for (int b = 0; b < nb; ++b) {
        const unsigned zm = zp[(size_t)b * n_paths];
        const unsigned x1 = xm & ~zm, z1 = zm & ~xm;
        const int na = __popc(x1), nz = __popc(z1);
        const bool ok = (xm | zm) == full;
        double wx = ok ? s_w[na * kMaxPath + nz] : 0.0;   // 0 when na = 0
        double wz = ok ? -s_w[nz * kMaxPath + na] : 0.0;  // 0 when nz = 0
        if (kProb) {
          const double s = s_s[b];
          wx *= s;
          wz *= s;
        }
#pragma unroll
        for (int l = 0; l < E; ++l) acc[l] += ((x1 >> l) & 1u) ? wx : (((z1 >> l) & 1u) ? wz : 0.0);
      }
      const double leaf = path_val[p];
#pragma unroll
      for (int l = 0; l < E; ++l)
        if (l < k) s_val[(size_t)tid * E + l] = leaf * acc[l];
    }
    __syncthreads();
    // ---- phase 2: (group, feature) sums in path order, then the groups in order
    const int np = min(kBgBlock, n_paths - p0);
    for (int c = tid; c < kBgGroups * F; c += kBgBlock) {
      const int g = c / F, f = c - g * F;
      const int t1 = min(np, (g + 1) * kBgGroup);
      double sum = 0.0;
      for (int t = g * kBgGroup; t < t1; ++t) {
        const int pos = s_pos[(size_t)t * fs + f];
        if (pos != 0xFF) sum += s_val[(size_t)t * E + pos];
      }
      s_part[g * fs + f] = sum;
    }
    __syncthreads();
    for (int f = tid; f < F; f += kBgBlock) {
      double tot = s_tot[f];
#pragma unroll
      for (int g = 0; g < kBgGroups; ++g) tot += s_part[g * fs + f];
      s_tot[f] = tot;
    }
    // (s_part is written again only after the next step's first barrier; s_tot[f] has one owner)
  }

  for (int f = tid; f < F; f += kBgBlock) {
    double v = s_tot[f];
    if (!first) v += phi[row * F + f];
    if (last) v /= n_background;
    phi[row * F + f] = v;
  }
}

template <int P, bool kProb>
int bg_launch(const float* X, int64_t n, int F, int64_t ldx, const PathElem* elems, const int32_t* path_ptr,
              const double* path_val, int n_paths, const uint16_t* zmask, const double* zmargin, int nb,
              const double* xmargin, int first, int last, int64_t n_background, double* phi, hipStream_t stream) {
  const size_t lds = bg_lds(F, P, kProb ? nb : 0);
  if (lds > 150 * 1024) return -5;
  static size_t attr_set = 48 * 1024;
  if (lds > attr_set) {
    CK(hipFuncSetAttribute((const void*)k_shapbg<P, kProb>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = lds;
  }
  hipLaunchKernelGGL((k_shapbg<P, kProb>), dim3((unsigned)n), dim3(kBgBlock), lds, stream, X, n, F, ldx, elems,
                     path_ptr, path_val, n_paths, zmask, zmargin, nb, xmargin, first, last, (double)n_background, phi);
  CK_LAUNCH();
  return 0;
}
}  // namespace

// Widest X and largest background tile the interventional kernel takes.
COBALT_API int cobalt_shapbg_max_f() { return kBgMaxF; }
COBALT_API int cobalt_shapbg_max_tile() { return kBgMaxTile; }

// masks [n, n_paths] uint16 (may be null) and margins [n] float64 of the rows X [n, F] (row stride ldx).
// -3: a path longer than kMaxPath - 1 features; -4: too many rows for one launch; -5: F outside
// 1..kBgMaxF; -6: a null buffer. Nothing is launched on an error.
COBALT_API int cobalt_shapbg_masks(const float* X, int64_t n, int F, int64_t ldx, const void* elems,
                                   const int32_t* path_ptr, const double* path_val, int n_paths, int max_len,
                                   double base_margin, uint16_t* masks, double* margins, hipStream_t stream) {
  if (n <= 0) return 0;
  if (F < 1 || F > kBgMaxF) return -5;
  if (max_len + 1 > kMaxPath) return -3;
  if (n > 0x7FFFFFFF) return -4;
  if (n_paths < 0 || ldx < F) return -6;
  if (!X || !margins || (n_paths > 0 && (!path_ptr || !path_val)) || (max_len > 0 && !elems)) return -6;
  hipLaunchKernelGGL(k_shapbg_masks, dim3((unsigned)n), dim3(kBgBlock), (size_t)bg_pos_stride(F) * sizeof(float),
                     stream, X, n, F, ldx, static_cast<const PathElem*>(elems), path_ptr, path_val, n_paths,
                     base_margin, masks, margins);
  CK_LAUNCH();
  return 0;
}

// One background tile of nb rows (masks zmask [nb, n_paths], margins zmargin [nb]) into phi [n, F] float64
// for the rows X [n, F]: `first` stores, otherwise the tile is added to phi; `last` divides by n_background.
// xmargin [n]: the rows' margins, selects the probability rescaling (null: margin space).
// Error codes as cobalt_shapbg_masks, and -7: nb outside 1..kBgMaxTile.
COBALT_API int cobalt_treeshap_interventional(const float* X, int64_t n, int F, int64_t ldx, const void* elems,
                                              const int32_t* path_ptr, const double* path_val, int n_paths,
                                              int max_len, const uint16_t* zmask, const double* zmargin, int nb,
                                              const double* xmargin, int first, int last, int64_t n_background,
                                              double* phi, hipStream_t stream) {
  if (n <= 0) return 0;
  if (F < 1 || F > kBgMaxF) return -5;
  if (max_len + 1 > kMaxPath) return -3;
  if (n > 0x7FFFFFFF) return -4;
  if (nb < 1 || nb > kBgMaxTile || n_background < nb) return -7;
  if (n_paths < 0 || ldx < F) return -6;
  if (!X || !phi || !zmargin || (n_paths > 0 && (!path_ptr || !path_val || !zmask)) || (max_len > 0 && !elems))
    return -6;
  const PathElem* pe = static_cast<const PathElem*>(elems);
  if (max_len + 1 <= 8) {
    if (xmargin)
      return bg_launch<8, true>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, zmask, zmargin, nb, xmargin, first,
                                last, n_background, phi, stream);
    return bg_launch<8, false>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, zmask, zmargin, nb, xmargin, first,
                               last, n_background, phi, stream);
  }
  if (xmargin)
    return bg_launch<kMaxPath, true>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, zmask, zmargin, nb, xmargin,
                                     first, last, n_background, phi, stream);
  return bg_launch<kMaxPath, false>(X, n, F, ldx, pe, path_ptr, path_val, n_paths, zmask, zmargin, nb, xmargin,
                                    first, last, n_background, phi, stream);
}
