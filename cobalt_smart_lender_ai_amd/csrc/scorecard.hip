// The WoE points scorecard on the GPU (gfx950): models/scorecard.py holds the definitions (scorecard_encode_host,
// scorecard_newton_host, scorecard_score_host) and is the CPU path.
//
// Layout, shared with bincount.hip: feature f has K_f interior edges (finite, strictly increasing, checked by the
// caller) and K_f + 2 cells; cell_ptr[f] is its first cell in the concatenated tables (cell_ptr[F] = all cells),
// so its edges start at cell_ptr[f] - 2 f of `edges`. A value x goes to cell #{i : z[i] < x}, NaN to cell K_f + 1.
//
//  k_sc_encode   float32 X (rows ldx apart) -> uint8 codes [N, F]: one element per lane, the edges in LDS, the
//                search of bincount.hip. Exact.
//  k_sc_newton   one Newton pass of the logistic regression on the WoE values: codes, y, w, beta -> per-wave
//                partials of the loss, the gradient and the upper tile triangle of the Hessian; k_sc_reduce adds
//                the partials in a fixed order and writes loss, grad [P] and the mirrored hess [P, P], P = F + 1.
//                 * A wave walks chunks of 64 rows. Phase A, one lane per row: eta in feature order, e =
//                   exp(-|eta|) once, p and q both from e, the row's s = w p q, g = w r and its loss term. s and
//                   g go to LDS.
//                 * Phase B, 16 steps of v_mfma_f64_16x16x4_f64 with the rows as the K dimension: lane l holds
//                   row l >> 4 of the step and column 16 t + (l & 15) of tile t, which is at once the A operand
//                   (Z~^T) of row tile t and, times s, the B operand (W Z~) of column tile t. Column P of B is
//                   g, so the gradient is one more column of D = Z~^T [W Z~ | g]. Only tiles tj >= ti are
//                   computed. C/D of the f64 instruction: col = lane & 15, row = (lane >> 4) + 4 reg.
//                 * Rows past N (and chunks past the block's share) have s = g = 0 and a finite z (code 0), so
//                   they add exact zeros; so does the tail of a 4-row step.
//                 * No floating-point atomics. The grid is a function of N alone, every wave writes one partial,
//                   the reduce adds them in index order: the same input gives the same bits on every run.
//  k_sc_score    float32 X -> float64 margin (beta_0 plus the host's per-cell contributions, added in feature
//                order: the host's bits), the int32 integer-points score and the int32 [N, top] reason indices
//                (largest shortfall first, ties to the lower feature, -1 once the shortfall is 0). One thread
//                per row, no cross-lane arithmetic.
//
// Refusals come before any launch: -1 F outside 1 .. kScMaxFeatures, -2 ldx < F, -3 n < 0, -4 a missing pointer,
// -5 a cell_ptr that does not start at 0, gives a feature fewer than 2 or more than 256 cells, or more than
// kScMaxCells in all, -6 top outside 0 .. kScMaxTop, -7 a workspace that is too small. n == 0 launches nothing.
#include "common.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kScMaxFeatures = 63;
constexpr int kScMaxCells = 8192;
constexpr int kScMaxFeatureCells = 256;  // codes are uint8
constexpr int kScMaxTop = 8;
constexpr int kScBlock = 256;
constexpr int kScWaves = kScBlock / kWave;
constexpr int kScEncTileRows = 512;
constexpr int kScChunkRows = kWave;      // rows of one phase A / phase B round of a wave
constexpr int kScBlockChunks = 16;       // chunks of a block until the grid reaches kScMaxBlocks
constexpr int kScMaxBlocks = 512;
constexpr int kScPartPad = 16;           // doubles after a partial's tiles: the loss, then zeros
constexpr int kScRedElems = 16, kScRedSlices = 16;

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int sc_edges_below(const float* z, int K, float x) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (z[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__host__ __device__ constexpr int sc_tiles(int PT, int QT) { return PT * QT - PT * (PT - 1) / 2; }

int sc_check_table(const int32_t* cp, int F) {
  if (F < 1 || F > kScMaxFeatures) return -1;
  if (cp == nullptr) return -4;
  if (cp[0] != 0) return -5;
  for (int f = 0; f < F; ++f) {
    const int64_t c = (int64_t)cp[f + 1] - cp[f];
    if (c < 2 || c > kScMaxFeatureCells) return -5;
  }
  return cp[F] > kScMaxCells ? -5 : 0;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------- encode
__global__ __launch_bounds__(kScBlock) void k_sc_encode(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                        const float* __restrict__ edges,
                                                        const int32_t* __restrict__ cell_ptr,
                                                        uint8_t* __restrict__ codes) {
  extern __shared__ uint32_t s_enc[];
  int32_t* s_ptr = reinterpret_cast<int32_t*>(s_enc);       // [F + 1]
  float* s_edges = reinterpret_cast<float*>(s_enc + F + 1);  // [cells - 2 F]
  const int tid = threadIdx.x;
  const int nedges = cell_ptr[F] - 2 * F;
  for (int i = tid; i <= F; i += kScBlock) s_ptr[i] = cell_ptr[i];
  for (int i = tid; i < nedges; i += kScBlock) s_edges[i] = edges[i];
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * kScEncTileRows;
  const int rows = (int)min((int64_t)kScEncTileRows, n - r0);
  const int ne = rows * F;
  for (int e = tid; e < ne; e += kScBlock) {
    const int row = e / F, f = e - row * F;
    const float x = X[(r0 + row) * ldx + f];
    const int first = s_ptr[f];
    const int K = s_ptr[f + 1] - first - 2;
    const int cell = (x != x) ? K + 1 : sc_edges_below(s_edges + (first - 2 * f), K, x);
    codes[r0 * F + e] = (uint8_t)cell;
  }
}

// ---------------------------------------------------------------------------------------------------- newton
// LDS: tab [cells] doubles | beta [F + 1] doubles | s, g [waves][64] doubles | ptr [F + 1] ints | codes [waves]
// [cw] words, cw = 16 F (64 rows of F bytes).
__host__ __device__ __forceinline__ size_t sc_newton_lds(int F, int cells) {
  return (size_t)(cells + (F + 1) + 2 * kScWaves * kScChunkRows) * sizeof(double) +
         (size_t)((F + 2) / 2 * 2 + kScWaves * 16 * F) * sizeof(uint32_t);
}

template <int PT, int QT>
__global__ __launch_bounds__(kScBlock) void k_sc_newton(const uint8_t* __restrict__ codes, int64_t n, int F,
                                                        const int32_t* __restrict__ cell_ptr,
                                                        const double* __restrict__ tab,
                                                        const float* __restrict__ y, const double* __restrict__ w,
                                                        const double* __restrict__ beta, int chunks_per_block,
                                                        double* __restrict__ part) {
  extern __shared__ double s_nw[];
  constexpr int NT = sc_tiles(PT, QT);
  const int cells = cell_ptr[F];
  const int P = F + 1;
  double* s_tab = s_nw;
  double* s_beta = s_tab + cells;
  double* s_s = s_beta + P;
  double* s_g = s_s + kScWaves * kScChunkRows;
  int32_t* s_ptr = reinterpret_cast<int32_t*>(s_g + kScWaves * kScChunkRows);
  uint32_t* s_codes = reinterpret_cast<uint32_t*>(s_ptr + (F + 2) / 2 * 2);
  const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
  for (int i = tid; i < cells; i += kScBlock) s_tab[i] = tab[i];
  for (int i = tid; i < P; i += kScBlock) s_beta[i] = beta[i];
  for (int i = tid; i <= F; i += kScBlock) s_ptr[i] = cell_ptr[i];
  __syncthreads();

  const int cw = 16 * F;  // words of a chunk's codes
  uint32_t* my_codes = s_codes + wv * cw;
  const uint8_t* my_bytes = reinterpret_cast<const uint8_t*>(my_codes);
  double* my_s = s_s + wv * kScChunkRows;
  double* my_g = s_g + wv * kScChunkRows;
  const int64_t nbytes = n * (int64_t)F;

  // the columns 16 t + (lane & 15) of this lane: 0 the intercept, 1 .. F a feature, P the gradient column of B
  int col_first[QT], col_last[QT];  // first cell and last cell index of the column's feature (when it is one)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int j = 16 * t + (lane & 15);
    const bool feat = j >= 1 && j <= F;
    col_first[t] = feat ? s_ptr[j - 1] : 0;
    col_last[t] = feat ? s_ptr[j] - s_ptr[j - 1] - 1 : 0;
  }

  d4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  double loss = 0.0;

  const int64_t nchunks = (n + kScChunkRows - 1) / kScChunkRows;
  const int64_t c_begin = (int64_t)blockIdx.x * chunks_per_block;
  const int64_t c_end = min(c_begin + chunks_per_block, nchunks);
  const int rounds = (chunks_per_block + kScWaves - 1) / kScWaves;  // block-uniform: every wave meets every barrier
  for (int rd = 0; rd < rounds; ++rd) {
    const int64_t chunk = c_begin + (int64_t)rd * kScWaves + wv;
    const bool live = chunk < c_end;
    const int64_t b0 = chunk * kScChunkRows * (int64_t)F;  // first byte of the chunk: a multiple of 64
    // stage the chunk's codes: whole words while they lie inside the matrix, single bytes at its end, zeros past it
    for (int i = lane; i < cw; i += kWave) {
      const int64_t b = b0 + 4 * (int64_t)i;
      uint32_t v = 0u;
      if (live) {
        if (b + 4 <= nbytes) {
          v = *reinterpret_cast<const uint32_t*>(codes + b);
        } else {
          for (int k = 0; k < 4; ++k)
            if (b + k < nbytes) v |= (uint32_t)codes[b + k] << (8 * k);
        }
      }
      my_codes[i] = v;
    }
    __syncthreads();

    {  // phase A: lane = row
      const int64_t row = chunk * kScChunkRows + lane;
      const bool valid = live && row < n;
      double eta = s_beta[0];
      for (int f = 0; f < F; ++f) {
        const int first = s_ptr[f];
        const int c = min((int)my_bytes[lane * F + f], s_ptr[f + 1] - first - 1);
        eta = eta + s_beta[f + 1] * s_tab[first + c];
      }
      const double e = exp(-fabs(eta));
      const double inv = 1.0 / (1.0 + e);
      const double big = inv, small = e * inv;
      const double p = eta >= 0.0 ? big : small;
      const double q = eta >= 0.0 ? small : big;
      const bool pos = valid && y[row] > 0.5f;
      const double wr = valid ? (w ? w[row] : 1.0) : 0.0;
      const double r = pos ? -q : p;
      my_s[lane] = wr * (p * q);
      my_g[lane] = wr * r;
      loss += wr * (log1p(e) + fmax(eta, 0.0) - (pos ? eta : 0.0));
    }
    __syncthreads();

    // phase B: 16 K-steps of 4 rows
#pragma unroll 2
    for (int kk = 0; kk < kScChunkRows / 4; ++kk) {
      const int rr = 4 * kk + (lane >> 4);
      const double srow = my_s[rr], grow = my_g[rr];
      double a[QT], b[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const int j = 16 * t + (lane & 15);
        double z = 0.0;
        if (j == 0) {
          z = 1.0;
        } else if (j <= F) {
          const int c = min((int)my_bytes[rr * F + (j - 1)], col_last[t]);
          z = s_tab[col_first[t] + c];
        }
        a[t] = z;
        b[t] = j == P ? grow : z * srow;
      }
#pragma unroll
      for (int ti = 0; ti < PT; ++ti) {
#pragma unroll
        for (int tj = ti; tj < QT; ++tj) {
          constexpr int kRowStart[4] = {0, QT, 2 * QT - 1, 3 * QT - 3};  // tiles before row tile ti
          const int t = kRowStart[ti] + (tj - ti);
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ti], b[tj], acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // the next round overwrites this wave's codes, s and g
  }

  // the wave's partial: [tile][reg][lane], then the loss and zeros
  constexpr int E = NT * 256;
  double* out = part + ((int64_t)blockIdx.x * kScWaves + wv) * (E + kScPartPad);
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(i * 4 + r) * kWave + lane] = acc[i][r];
  }
  const double total = wave_total_f64(loss);
  if (lane < kScPartPad - 1) out[E + 1 + lane] = 0.0;
  if (lane == kWave - 1) out[E] = total;
}

// Block b: the elements 16 b .. 16 b + 15 of the partials (pitch doubles apart, nparts of them). Thread (element
// tid & 15, slice tid >> 4) adds the partials slice, slice + 16, ... in index order; slice 0 then adds the 16 slice
// sums in slice order and writes the element where it belongs in out = [loss | grad P | hess P x P].
__global__ __launch_bounds__(kScRedElems * kScRedSlices) void k_sc_reduce(const double* __restrict__ part, int nparts,
                                                                         int pitch, int PT, int QT, int P,
                                                                         double* __restrict__ out) {
  __shared__ double s[kScRedSlices][kScRedElems];
  const int el = threadIdx.x & (kScRedElems - 1), sl = threadIdx.x / kScRedElems;
  const int e = blockIdx.x * kScRedElems + el;
  double v = 0.0;
  for (int p = sl; p < nparts; p += kScRedSlices) v += part[(int64_t)p * pitch + e];
  s[sl][el] = v;
  __syncthreads();
  if (sl != 0) return;
  for (int k = 1; k < kScRedSlices; ++k) v += s[k][el];
  const int E = sc_tiles(PT, QT) * 256;
  if (e >= E) {
    if (e == E) out[0] = v;
    return;
  }
  int tile = e >> 8, ti = 0;
  while (tile >= QT - ti) {  // row tile ti has the column tiles ti .. QT - 1
    tile -= QT - ti;
    ++ti;
  }
  const int tj = ti + tile;
  const int reg = (e >> 6) & 3, lane = e & 63;
  const int i = 16 * ti + (lane >> 4) + 4 * reg, j = 16 * tj + (lane & 15);
  if (i >= P) return;
  double* grad = out + 1;
  double* hess = out + 1 + P;
  if (j == P) {
    grad[i] = v;
  } else if (j < P && i <= j) {  // one triangle, mirrored
    hess[(int64_t)i * P + j] = v;
    hess[(int64_t)j * P + i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------- score
template <int TOP>
__global__ __launch_bounds__(kScBlock) void k_sc_score(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                       const float* __restrict__ edges,
                                                       const int32_t* __restrict__ cell_ptr, double beta0,
                                                       const double* __restrict__ contrib,
                                                       const int32_t* __restrict__ ipoints,
                                                       const double* __restrict__ shortfall,
                                                       double* __restrict__ margin, int32_t* __restrict__ iscore,
                                                       int32_t* __restrict__ reasons) {
  extern __shared__ uint32_t s_sc[];
  int32_t* s_ptr = reinterpret_cast<int32_t*>(s_sc);
  float* s_edges = reinterpret_cast<float*>(s_sc + F + 1);
  const int tid = threadIdx.x;
  const int nedges = cell_ptr[F] - 2 * F;
  for (int i = tid; i <= F; i += kScBlock) s_ptr[i] = cell_ptr[i];
  for (int i = tid; i < nedges; i += kScBlock) s_edges[i] = edges[i];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * kScBlock + tid;
  if (row >= n) return;
  double m = beta0;
  int32_t pts = 0;
  double bv[TOP > 0 ? TOP : 1];
  int32_t bi[TOP > 0 ? TOP : 1];
#pragma unroll
  for (int k = 0; k < TOP; ++k) {
    bv[k] = 0.0;
    bi[k] = -1;
  }
  for (int f = 0; f < F; ++f) {
    const float x = X[row * ldx + f];
    const int first = s_ptr[f];
    const int K = s_ptr[f + 1] - first - 2;
    const int cell = first + ((x != x) ? K + 1 : sc_edges_below(s_edges + (first - 2 * f), K, x));
    m = m + contrib[cell];
    pts += ipoints[cell];
    if constexpr (TOP > 0) {
      double v = shortfall[cell];
      int32_t idx = f;
      bool carry = false;  // once inserted, the displaced entries move down one place
#pragma unroll
      for (int k = 0; k < TOP; ++k) {
        if (carry || v > bv[k]) {
          const double tv = bv[k];
          const int32_t tix = bi[k];
          bv[k] = v;
          bi[k] = idx;
          v = tv;
          idx = tix;
          carry = true;
        }
      }
    }
  }
  margin[row] = m;
  iscore[row] = pts;
#pragma unroll
  for (int k = 0; k < TOP; ++k) reasons[row * TOP + k] = bi[k];
}

// ---------------------------------------------------------------------------------------------------- C ABI
COBALT_API int cobalt_sc_max_features() { return kScMaxFeatures; }
COBALT_API int cobalt_sc_max_cells() { return kScMaxCells; }
COBALT_API int cobalt_sc_max_top() { return kScMaxTop; }
COBALT_API int cobalt_sc_encode_tile_rows() { return kScEncTileRows; }
COBALT_API int cobalt_sc_newton_block_rows() { return kScBlockChunks * kScChunkRows; }

COBALT_API int cobalt_sc_encode(const float* X, int64_t n, int F, int64_t ldx, const float* edges,
                                const int32_t* cell_ptr_host, const int32_t* cell_ptr, uint8_t* codes,
                                hipStream_t stream) {
  const int rc = sc_check_table(cell_ptr_host, F);
  if (rc) return rc;
  if (ldx < F) return -2;
  if (n < 0) return -3;
  if (cell_ptr == nullptr || (edges == nullptr && cell_ptr_host[F] > 2 * F)) return -4;
  if (n == 0) return 0;
  if (X == nullptr || codes == nullptr) return -4;
  const int64_t blocks = (n + kScEncTileRows - 1) / kScEncTileRows;
  if (blocks > 0x7fffffff) return -3;
  const size_t lds = (size_t)(F + 1 + cell_ptr_host[F] - 2 * F) * sizeof(uint32_t);
  hipLaunchKernelGGL(k_sc_encode, dim3((unsigned)blocks), dim3(kScBlock), lds, stream, X, n, F, ldx, edges, cell_ptr,
                     codes);
  CK_LAUNCH();
  return 0;
}

namespace {
struct ScPlan {
  int PT, QT, chunks_per_block, blocks, pitch;
};
ScPlan sc_plan(int64_t n, int F) {
  ScPlan p;
  p.PT = (F + 1 + 15) / 16;
  p.QT = (F + 2 + 15) / 16;
  const int64_t nchunks = (n + kScChunkRows - 1) / kScChunkRows;
  p.chunks_per_block = (int)std::max<int64_t>(kScBlockChunks, (nchunks + kScMaxBlocks - 1) / kScMaxBlocks);
  p.blocks = (int)((nchunks + p.chunks_per_block - 1) / p.chunks_per_block);
  p.pitch = sc_tiles(p.PT, p.QT) * 256 + kScPartPad;
  return p;
}

template <int PT, int QT>
int sc_launch_newton(const ScPlan& pl, size_t lds, hipStream_t stream, const uint8_t* codes, int64_t n, int F,
                     const int32_t* cell_ptr, const double* tab, const float* y, const double* w, const double* beta,
                     double* part) {
  if (lds > 64 * 1024)
    CK(hipFuncSetAttribute((const void*)k_sc_newton<PT, QT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_sc_newton<PT, QT>), dim3((unsigned)pl.blocks), dim3(kScBlock), lds, stream, codes, n, F,
                     cell_ptr, tab, y, w, beta, pl.chunks_per_block, part);
  CK_LAUNCH();
  return 0;
}
}  // namespace

// Bytes of the partials of one pass over n rows of F features (0 for n == 0); negative: a refusal.
COBALT_API int64_t cobalt_sc_newton_workspace_bytes(int64_t n, int F) {
  if (F < 1 || F > kScMaxFeatures) return -1;
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  const ScPlan p = sc_plan(n, F);
  return (int64_t)p.blocks * kScWaves * p.pitch * (int64_t)sizeof(double);
}

// codes: uint8 [n, F] contiguous; tab: float64 [cells]; y: float32 [n]; w: float64 [n] or null (1 per row); beta:
// float64 [F + 1]; out: float64 [1 + P + P P] = loss, grad, hess (written, not added to; zeros when n == 0 are the
// caller's). All on the device but cell_ptr_host.
COBALT_API int cobalt_sc_newton(const uint8_t* codes, int64_t n, int F, const int32_t* cell_ptr_host,
                                const int32_t* cell_ptr, const double* tab, const float* y, const double* w,
                                const double* beta, double* workspace, int64_t workspace_bytes, double* out,
                                hipStream_t stream) {
  const int rc = sc_check_table(cell_ptr_host, F);
  if (rc) return rc;
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  if (cell_ptr == nullptr || tab == nullptr || beta == nullptr || out == nullptr) return -4;
  if (n == 0) return 0;
  if (codes == nullptr || y == nullptr || workspace == nullptr) return -4;
  const ScPlan pl = sc_plan(n, F);
  if (workspace_bytes < (int64_t)pl.blocks * kScWaves * pl.pitch * (int64_t)sizeof(double)) return -7;
  const size_t lds = sc_newton_lds(F, cell_ptr_host[F]);
  int r = 0;
#define SC_CASE(PT_, QT_)                                                                                         \
  if (pl.PT == PT_ && pl.QT == QT_)                                                                               \
    r = sc_launch_newton<PT_, QT_>(pl, lds, stream, codes, n, F, cell_ptr, tab, y, w, beta, workspace);           \
  else
  SC_CASE(1, 1) SC_CASE(1, 2) SC_CASE(2, 2) SC_CASE(2, 3) SC_CASE(3, 3) SC_CASE(3, 4) SC_CASE(4, 4) SC_CASE(4, 5)
  return -1;
#undef SC_CASE
  if (r) return r;
  const int P = F + 1;
  hipLaunchKernelGGL(k_sc_reduce, dim3((unsigned)(pl.pitch / kScRedElems)), dim3(kScRedElems * kScRedSlices), 0,
                     stream, workspace, pl.blocks * kScWaves, pl.pitch, pl.PT, pl.QT, P, out);
  CK_LAUNCH();
  return 0;
}

// contrib, shortfall: float64 [cells]; ipoints: int32 [cells]; margin: float64 [n]; iscore: int32 [n]; reasons:
// int32 [n, top] (may be null when top == 0).
COBALT_API int cobalt_sc_score(const float* X, int64_t n, int F, int64_t ldx, const float* edges,
                               const int32_t* cell_ptr_host, const int32_t* cell_ptr, double beta0,
                               const double* contrib, const int32_t* ipoints, const double* shortfall, int top,
                               double* margin, int32_t* iscore, int32_t* reasons, hipStream_t stream) {
  const int rc = sc_check_table(cell_ptr_host, F);
  if (rc) return rc;
  if (ldx < F) return -2;
  if (n < 0) return -3;
  if (top < 0 || top > kScMaxTop) return -6;
  if (cell_ptr == nullptr || contrib == nullptr || ipoints == nullptr || shortfall == nullptr) return -4;
  if (edges == nullptr && cell_ptr_host[F] > 2 * F) return -4;
  if (n == 0) return 0;
  if (X == nullptr || margin == nullptr || iscore == nullptr || (top > 0 && reasons == nullptr)) return -4;
  const int64_t blocks = (n + kScBlock - 1) / kScBlock;
  if (blocks > 0x7fffffff) return -3;
  const size_t lds = (size_t)(F + 1 + cell_ptr_host[F] - 2 * F) * sizeof(uint32_t);
#define SC_TOP(T_)                                                                                                 \
  case T_:                                                                                                         \
    hipLaunchKernelGGL(k_sc_score<T_>, dim3((unsigned)blocks), dim3(kScBlock), lds, stream, X, n, F, ldx, edges,    \
                       cell_ptr, beta0, contrib, ipoints, shortfall, margin, iscore, reasons);                     \
    break;
  switch (top) {
    SC_TOP(0) SC_TOP(1) SC_TOP(2) SC_TOP(3) SC_TOP(4) SC_TOP(5) SC_TOP(6) SC_TOP(7) SC_TOP(8)
  }
#undef SC_TOP
  CK_LAUNCH();
  return 0;
}
