// Pairwise-complete correlation moments on the GPU (gfx950): ops/corr_ops.py holds the definition
// (pair_moments_host) and is the CPU path.
//
// Input: float32 X (rows ldx apart, column slices are read in place) and a float64 centre mu [F]. A value is
// present iff it is finite; a present value gives c = (double)x - mu[f] and m = 1, a missing one c = m = 0. For
// every ordered pair (i, j)
//     n[i,j] = sum m_i m_j (int64)   A[i,j] = sum c_i m_j   Q[i,j] = sum c_i^2 m_j   P[i,j] = sum c_i c_j
// which is [C | C.C | M]^T [C | M] without the two blocks nobody reads.
//
//  k_corr_colsum   per block and column the float64 sum and the count of the present values (the wrapper's centre
//                  is their mean); the caller adds the blocks' partials.
//  k_corr_moments  FT = ceil(F / 16) column tiles. A block of four waves walks chunks of 64 rows: all threads stage
//                  the chunk's c and m as doubles in LDS (columns past F and rows past N as zeros), so X is read
//                  from HBM once. Then 16 steps of v_mfma_f64_16x16x4_f64 with the rows as the K dimension: lane l
//                  holds row l >> 4 of the step and column 16 t + (l & 15) of tile t, read from LDS, which is at
//                  once an A operand (as row tile) and a B operand (as column tile). C/D of the f64 instruction:
//                  col = lane & 15, row = (lane >> 4) + 4 reg.
//                   * The row tiles are split over the waves: wave w has row tile w and, from FT = 5 on, row tile
//                     FT - 1 - w when that is 4 or more. For each of its row tiles ti it holds A and Q for all
//                     column tiles and P and n for tj >= ti; the P / n tiles of both row tiles share one list of
//                     FT (+ 1 with two row tiles) slots whose tile offsets are wave-uniform values.
//                   * Rows past N and the tail of a 4-row step have c = m = 0: exact zeros. n goes through the same
//                     MFMA (exact below 2^53) and is converted in the reduce.
//                   * No floating-point atomics. The grid is a function of (N, F) alone, every block writes one
//                     partial ([tile][reg][lane]), k_corr_reduce adds the partials in index order, mirrors P and n
//                     and writes the four [F, F] tables: the same input gives the same bits on every call.
//
// Refusals come before any launch: -1 F outside 1 .. kCorrMaxFeatures, -2 ldx < F, -3 n < 0 (or above 2^40), -4 a
// missing pointer, -7 a workspace that is too small. n == 0 launches no kernel and writes zeros.
#include "common.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kCorrMaxFeatures = 128;
constexpr int kCorrBlock = 256;
constexpr int kCorrWaves = kCorrBlock / kWave;
constexpr int kCorrChunkRows = 64;    // rows staged in LDS at a time
constexpr int kCorrBlockChunks = 4;   // chunks of a block until the grid reaches kCorrMaxBlocks
constexpr int kCorrMaxBlocks = 512;
constexpr int kCorrRedElems = 16, kCorrRedSlices = 16;
constexpr int kCorrSumCols = 128;     // pitch of a block's column sums

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int corr_tri(int FT) { return FT * (FT + 1) / 2; }
__host__ __device__ constexpr int corr_tiles(int FT) { return 2 * FT * FT + 2 * corr_tri(FT); }
// tiles of the upper triangle before (ti, tj), tj >= ti
__host__ __device__ constexpr int corr_tri_at(int FT, int ti, int tj) { return ti * FT - ti * (ti - 1) / 2 + (tj - ti); }
// doubles between two staged rows: an odd number of 128-byte groups, so the four rows of a step tile the 64 banks
__host__ __device__ constexpr int corr_ldw(int FT) { return 16 * (FT | 1); }
__host__ __device__ constexpr size_t corr_lds(int FT) {
  return (size_t)(2 * kCorrChunkRows * corr_ldw(FT) + 16 * FT) * sizeof(double);
}

__device__ __forceinline__ bool corr_present(float x) { return fabsf(x) < INFINITY; }

struct CorrPlan {
  int FT, chunks_per_block, blocks;
  int64_t pitch;  // doubles of one block's partial
};
CorrPlan corr_plan(int64_t n, int F) {
  CorrPlan p;
  p.FT = (F + 15) / 16;
  const int64_t nchunks = (n + kCorrChunkRows - 1) / kCorrChunkRows;
  p.chunks_per_block = (int)std::max<int64_t>(kCorrBlockChunks, (nchunks + kCorrMaxBlocks - 1) / kCorrMaxBlocks);
  p.blocks = (int)((nchunks + p.chunks_per_block - 1) / p.chunks_per_block);
  p.pitch = (int64_t)corr_tiles(p.FT) * 256;
  return p;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------- column sums
// Thread (column tid & 127, row lane tid >> 7) adds its rows of the block's share in row order; the two row lanes
// are added in lane order. sums, counts: [blocks][kCorrSumCols].
__global__ __launch_bounds__(kCorrBlock) void k_corr_colsum(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                            int chunks_per_block, double* __restrict__ sums,
                                                            int64_t* __restrict__ counts) {
  __shared__ double s_sum[kCorrSumCols];
  __shared__ int64_t s_cnt[kCorrSumCols];
  const int col = threadIdx.x & (kCorrSumCols - 1), rl = threadIdx.x / kCorrSumCols;
  const int64_t r0 = (int64_t)blockIdx.x * chunks_per_block * kCorrChunkRows;
  const int64_t r1 = min(r0 + (int64_t)chunks_per_block * kCorrChunkRows, n);
  double s = 0.0;
  int64_t c = 0;
  if (col < F) {
    for (int64_t r = r0 + rl; r < r1; r += kCorrBlock / kCorrSumCols) {
      const float x = X[r * ldx + col];
      if (corr_present(x)) {
        s += (double)x;
        ++c;
      }
    }
  }
  if (rl == 1) {
    s_sum[col] = s;
    s_cnt[col] = c;
  }
  __syncthreads();
  if (rl == 0) {
    sums[(int64_t)blockIdx.x * kCorrSumCols + col] = s + s_sum[col];
    counts[(int64_t)blockIdx.x * kCorrSumCols + col] = c + s_cnt[col];
  }
}

// ---------------------------------------------------------------------------------------------------- moments
// LDS: c [64][ldw] doubles | m [64][ldw] doubles | mu [16 FT] doubles.
template <int FT>
__global__ __launch_bounds__(kCorrBlock) void k_corr_moments(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                             const double* __restrict__ mu, int chunks_per_block,
                                                             double* __restrict__ part) {
  extern __shared__ double s_corr[];
  constexpr int LDW = corr_ldw(FT), FW = 16 * FT;
  constexpr bool kTwo = FT > kCorrWaves;       // some wave has a second row tile
  constexpr int NS = FT + (kTwo ? 1 : 0);      // P / n slots of a wave
  double* s_c = s_corr;
  double* s_m = s_c + kCorrChunkRows * LDW;
  double* s_mu = s_m + kCorrChunkRows * LDW;
  const int tid = threadIdx.x, lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
  for (int i = tid; i < FW; i += kCorrBlock) s_mu[i] = i < F ? mu[i] : 0.0;

  // this wave's row tiles and the (row tile, column tile) of its P / n slots, as LDS offsets
  const int ti0 = wv, ti1 = FT - 1 - wv;
  const bool has0 = ti0 < FT, has1 = kTwo && ti1 >= kCorrWaves;
  const int cnt0 = has0 ? FT - ti0 : 0, cnt1 = has1 ? FT - ti1 : 0;
  int sa[NS], sb[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool first = s < cnt0;
    const int ta = first ? ti0 : ti1;
    sa[s] = 16 * ta;
    sb[s] = 16 * (first ? ti0 + s : ti1 + (s - cnt0));
  }

  d4 accA0[FT], accQ0[FT], accA1[kTwo ? FT : 1], accQ1[kTwo ? FT : 1], accP[NS], accN[NS];
  const d4 zero = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int t = 0; t < FT; ++t) {
    accA0[t] = zero;
    accQ0[t] = zero;
    if (kTwo) {
      accA1[t] = zero;
      accQ1[t] = zero;
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    accP[s] = zero;
    accN[s] = zero;
  }

  const int64_t nchunks = (n + kCorrChunkRows - 1) / kCorrChunkRows;
  const int64_t c_begin = (int64_t)blockIdx.x * chunks_per_block;
  const int64_t c_end = min(c_begin + chunks_per_block, nchunks);
  for (int64_t chunk = c_begin; chunk < c_end; ++chunk) {  // block-uniform: every wave meets every barrier
    __syncthreads();  // the last chunk's operands are read (and, first, s_mu is written)
    const int64_t r0 = chunk * kCorrChunkRows;
    for (int e = tid; e < kCorrChunkRows * FW; e += kCorrBlock) {
      const int row = e / FW, col = e - row * FW;
      double c = 0.0, m = 0.0;
      if (col < F && r0 + row < n) {
        const float x = X[(r0 + row) * ldx + col];
        if (corr_present(x)) {
          c = (double)x - s_mu[col];
          m = 1.0;
        }
      }
      s_c[row * LDW + col] = c;
      s_m[row * LDW + col] = m;
    }
    __syncthreads();
    if (!has0) continue;

#pragma unroll 1
    for (int kk = 0; kk < kCorrChunkRows / 4; ++kk) {
      const int base = (4 * kk + (lane >> 4)) * LDW + (lane & 15);
      const double* pc = s_c + base;
      const double* pm = s_m + base;
      const double c0 = pc[16 * ti0];
      const double q0 = c0 * c0;
#pragma unroll
      for (int tj = 0; tj < FT; ++tj) {
        const double bm = pm[16 * tj];
        accA0[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, bm, accA0[tj], 0, 0, 0);
        accQ0[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(q0, bm, accQ0[tj], 0, 0, 0);
      }
      if (kTwo && has1) {
        const double c1 = pc[16 * ti1];
        const double q1 = c1 * c1;
#pragma unroll
        for (int tj = 0; tj < FT; ++tj) {
          const double bm = pm[16 * tj];
          accA1[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, bm, accA1[tj], 0, 0, 0);
          accQ1[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(q1, bm, accQ1[tj], 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s < cnt0 + cnt1) {
          accP[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(pc[sa[s]], pc[sb[s]], accP[s], 0, 0, 0);
          accN[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(pm[sa[s]], pm[sb[s]], accN[s], 0, 0, 0);
        }
      }
    }
  }
  if (!has0) return;

  // the block's partial: tiles A [FT][FT] | Q [FT][FT] | P upper triangle | n upper triangle, each [reg][lane]
  double* out = part + (int64_t)blockIdx.x * (corr_tiles(FT) * 256);
  auto put = [&](int tile, const d4& v) {
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(tile * 4 + r) * kWave + lane] = v[r];
  };
#pragma unroll
  for (int tj = 0; tj < FT; ++tj) {
    put(ti0 * FT + tj, accA0[tj]);
    put(FT * FT + ti0 * FT + tj, accQ0[tj]);
    if (kTwo && has1) {
      put(ti1 * FT + tj, accA1[tj]);
      put(FT * FT + ti1 * FT + tj, accQ1[tj]);
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s < cnt0 + cnt1) {
      const int t = corr_tri_at(FT, sa[s] / 16, sb[s] / 16);
      put(2 * FT * FT + t, accP[s]);
      put(2 * FT * FT + corr_tri(FT) + t, accN[s]);
    }
  }
}

// Block b: the elements 16 b .. 16 b + 15 of the partials (pitch doubles apart, nparts of them). Thread (element
// tid & 15, slice tid >> 4) adds the partials slice, slice + 16, ... in index order; slice 0 then adds the 16 slice
// sums in slice order and writes the element where it belongs (P and n: one triangle, mirrored).
__global__ __launch_bounds__(kCorrRedElems * kCorrRedSlices) void k_corr_reduce(const double* __restrict__ part,
                                                                             int nparts, int64_t pitch, int FT, int F,
                                                                             int64_t* __restrict__ n_out,
                                                                             double* __restrict__ a_out,
                                                                             double* __restrict__ q_out,
                                                                             double* __restrict__ p_out) {
  __shared__ double s[kCorrRedSlices][kCorrRedElems];
  const int el = threadIdx.x & (kCorrRedElems - 1), sl = threadIdx.x / kCorrRedElems;
  const int e = blockIdx.x * kCorrRedElems + el;
  double v = 0.0;
  for (int p = sl; p < nparts; p += kCorrRedSlices) v += part[(int64_t)p * pitch + e];
  s[sl][el] = v;
  __syncthreads();
  if (sl != 0) return;
  for (int k = 1; k < kCorrRedSlices; ++k) v += s[k][el];
  int tile = e >> 8;
  const int reg = (e >> 6) & 3, lane = e & 63;
  const int sq = FT * FT, tri = corr_tri(FT);
  int table, ti, tj;  // 0 A, 1 Q, 2 P, 3 n
  if (tile < 2 * sq) {
    table = tile / sq;
    tile -= table * sq;
    ti = tile / FT;
    tj = tile - ti * FT;
  } else {
    tile -= 2 * sq;
    table = 2 + tile / tri;
    tile -= (table - 2) * tri;
    ti = 0;
    while (tile >= FT - ti) {  // row tile ti has the column tiles ti .. FT - 1
      tile -= FT - ti;
      ++ti;
    }
    tj = ti + tile;
  }
  const int i = 16 * ti + (lane >> 4) + 4 * reg, j = 16 * tj + (lane & 15);
  if (i >= F || j >= F) return;
  const int64_t ij = (int64_t)i * F + j, ji = (int64_t)j * F + i;
  if (table == 0) {
    a_out[ij] = v;
  } else if (table == 1) {
    q_out[ij] = v;
  } else if (i <= j) {
    if (table == 2) {
      p_out[ij] = v;
      p_out[ji] = v;
    } else {
      n_out[ij] = (int64_t)v;
      n_out[ji] = (int64_t)v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- C ABI
COBALT_API int cobalt_corr_max_features() { return kCorrMaxFeatures; }
COBALT_API int cobalt_corr_chunk_rows() { return kCorrChunkRows; }
COBALT_API int cobalt_corr_block_rows() { return kCorrBlockChunks * kCorrChunkRows; }
COBALT_API int cobalt_corr_max_blocks() { return kCorrMaxBlocks; }

// Blocks of the grid over n rows (the rows of the column-sum partials); negative: a refusal.
COBALT_API int cobalt_corr_blocks(int64_t n) {
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  return corr_plan(n, 1).blocks;
}

// Bytes of the partials of one pass over n rows of F features (0 for n == 0); negative: a refusal.
COBALT_API int64_t cobalt_corr_workspace_bytes(int64_t n, int F) {
  if (F < 1 || F > kCorrMaxFeatures) return -1;
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  const CorrPlan p = corr_plan(n, F);
  return (int64_t)p.blocks * p.pitch * (int64_t)sizeof(double);
}

// sums: float64 [cobalt_corr_blocks(n)][128], counts: int64 of the same shape (columns past F: zeros); the column
// totals are their sums over the blocks.
COBALT_API int cobalt_corr_col_sums(const float* X, int64_t n, int F, int64_t ldx, double* sums, int64_t* counts,
                                    hipStream_t stream) {
  if (F < 1 || F > kCorrMaxFeatures) return -1;
  if (ldx < F) return -2;
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  if (n == 0) return 0;
  if (X == nullptr || sums == nullptr || counts == nullptr) return -4;
  const CorrPlan pl = corr_plan(n, F);
  hipLaunchKernelGGL(k_corr_colsum, dim3((unsigned)pl.blocks), dim3(kCorrBlock), 0, stream, X, n, F, ldx,
                     pl.chunks_per_block, sums, counts);
  CK_LAUNCH();
  return 0;
}

namespace {
template <int FT>
int corr_launch(const CorrPlan& pl, hipStream_t stream, const float* X, int64_t n, int F, int64_t ldx,
                const double* mu, double* part) {
  constexpr size_t lds = corr_lds(FT);
  if (lds > 64 * 1024)
    CK(hipFuncSetAttribute((const void*)k_corr_moments<FT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_corr_moments<FT>), dim3((unsigned)pl.blocks), dim3(kCorrBlock), lds, stream, X, n, F, ldx, mu,
                     pl.chunks_per_block, part);
  CK_LAUNCH();
  return 0;
}
}  // namespace

// X: float32 [n, F], rows ldx apart; mu: float64 [F]; n_out: int64 [F, F]; a_out, q_out, p_out: float64 [F, F]
// (written, not added to). All on the device.
COBALT_API int cobalt_corr_moments(const float* X, int64_t n, int F, int64_t ldx, const double* mu, double* workspace,
                                   int64_t workspace_bytes, int64_t* n_out, double* a_out, double* q_out,
                                   double* p_out, hipStream_t stream) {
  if (F < 1 || F > kCorrMaxFeatures) return -1;
  if (ldx < F) return -2;
  if (n < 0 || n > ((int64_t)1 << 40)) return -3;
  if (n_out == nullptr || a_out == nullptr || q_out == nullptr || p_out == nullptr) return -4;
  if (n == 0) {
    const size_t cells = (size_t)F * F;
    CK(hipMemsetAsync(n_out, 0, cells * sizeof(int64_t), stream));
    CK(hipMemsetAsync(a_out, 0, cells * sizeof(double), stream));
    CK(hipMemsetAsync(q_out, 0, cells * sizeof(double), stream));
    CK(hipMemsetAsync(p_out, 0, cells * sizeof(double), stream));
    return 0;
  }
  if (X == nullptr || mu == nullptr || workspace == nullptr) return -4;
  const CorrPlan pl = corr_plan(n, F);
  if (workspace_bytes < (int64_t)pl.blocks * pl.pitch * (int64_t)sizeof(double)) return -7;
  int r = 0;
  switch (pl.FT) {
#define CORR_CASE(FT_)                                                      \
  case FT_:                                                                 \
    r = corr_launch<FT_>(pl, stream, X, n, F, ldx, mu, workspace);          \
    break;
    CORR_CASE(1) CORR_CASE(2) CORR_CASE(3) CORR_CASE(4) CORR_CASE(5) CORR_CASE(6) CORR_CASE(7) CORR_CASE(8)
#undef CORR_CASE
    default:
      return -1;
  }
  if (r) return r;
  hipLaunchKernelGGL(k_corr_reduce, dim3((unsigned)(pl.pitch / kCorrRedElems)), dim3(kCorrRedElems * kCorrRedSlices),
                     0, stream, workspace, pl.blocks, pl.pitch, pl.FT, F, n_out, a_out, q_out, p_out);
  CK_LAUNCH();
  return 0;
}
