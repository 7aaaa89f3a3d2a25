// Accumulated local effects (ALE, Apley & Zhu) of a tree ensemble for one feature or a pair (gfx950): every
// row is moved only across the interval of the job's edges it already lies in and scored at that interval's
// corners -- x[f1] = z1[k - 1] (lo) and z1[k] (hi), everything else as in X; with a second feature the four
// corners of the cell (k, l) -- and the corner differences are summed per interval / cell.
//
// A client of the packed-forest block of forest_walk.h (ForestBlock), like pdp.hip and permimp.hip: one thread
// owns one row (features staged in LDS with the odd stride F | 1, rows past n as zeros), tiles of the forest
// are staged in LDS, leaf values are added in fp32 in tree order starting from base_margin, so every corner
// margin has the bits of predict_margin on the substituted row. The substitution is the select of pdp_walk.h
// on the value read from LDS: neither X nor the staged row is written.
//
// Design choices
//  * blockIdx.y is a job (one feature, or one pair), as in permimp.hip: "ALE of all 20 features" is one launch
//    per row chunk. A job is six int32 {f1, f2, off1, K1, off2, K2}: its edges are edges[off .. off + K] (K
//    intervals, K + 1 edges, concatenated for all jobs); 1-D has f2 = -1, K2 = 1. A call is all 1-D or all 2-D.
//  * The row finds its interval itself (ale_interval: k = clamp(#{i : z[i] < x}, 1, K), so z[k-1] < x <= z[k],
//    values outside the edges and +-inf are clamped, NaN lands in interval 1) by a binary search of the job's
//    edges, which are block-uniform and stay in cache; lo and hi are loaded into vector registers before the
//    tile loop. The corners are the chains of walk_tree_points: 2 chains per tree (1-D) or 4 = kWalk (2-D),
//    one fp32 accumulator per corner. Corner c = i1 + 2 i2 (i = 0: lo, 1: hi).
//  * No forked walk (one chain until the first split on f1 whose threshold lies inside the row's interval):
//    not measured, so not there.
//  * Grouped sums without floating-point atomics: k_ale_cells writes every row's cell (k - 1) * K2 + (l - 1)
//    (kAleNoCell for a NaN in a job's feature: such a row is walked like any other and enters no sum); the
//    caller sorts each row chunk's cells stably and passes `order` (chunk-local row indices, cell by cell) and
//    `seg_ptr` (where each cell starts). k_ale walks in natural row order; k_ale_reduce takes one block per
//    (job, cell), gathers the cell's contiguous segment of `order` and adds (w d_margin, w d_prob, w) in fp64
//    in a fixed order (thread i takes the entries i, i + 256, ... in index order, then a fixed LDS tree, as
//    k_pair_reduce). d_margin is the corner difference of the fp32 margins taken in fp64, d_prob that of
//    1 / (1 + exp(-m)) per corner in fp64. The same input gives the same bits on every run.
//  * Rows are processed in chunks of kAleChunkRows = 2^17 (which bounds the corner-margin workspace when the
//    per-row margins are not asked for: 4 C bytes per job and chunk row); chunk sums are added in chunk order.
#include "common.h"
#include "pdp_walk.h"
#include <algorithm>
#include <limits.h>

using namespace cobalt;

namespace {
constexpr int kAleBlock = 256;
constexpr int64_t kAleChunkRows = 1 << 17;
constexpr int kAleMaxIntervals = 4096;  // per axis
constexpr int kAleMaxCells = 1 << 16;   // K1 * K2 of a job
constexpr int kAleMaxJobs = 65535;      // gridDim.y
constexpr int kAleJobInts = 6;          // {f1, f2, off1, K1, off2, K2}
constexpr int32_t kAleNoCell = INT_MAX;

// Interval of x among the edges z[0 .. K]: clamp(#{i : z[i] < x}, 1, K) (searchsorted "left"). NaN: 1.
__device__ __forceinline__ int ale_interval(const float* __restrict__ z, int K, float x) {
  int lo = 0, hi = K + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (z[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return min(max(lo, 1), K);
}

struct AleJob {
  int f1, f2, off1, K1, off2, K2;
};
__device__ __forceinline__ AleJob load_job(const int32_t* __restrict__ jobs, int j) {
  const int32_t* d = jobs + (int64_t)j * kAleJobInts;
  return AleJob{d[0], d[1], d[2], d[3], d[4], d[5]};
}
}  // namespace

// cells[job][row] for the rows [0, n) (rows of ld entries): the row's interval / cell, kAleNoCell for NaN.
__global__ __launch_bounds__(kAleBlock) void k_ale_cells(const float* __restrict__ X, int64_t n, int64_t ldx,
                                                         const int32_t* __restrict__ jobs,
                                                         const float* __restrict__ edges,
                                                         int32_t* __restrict__ cells, int64_t ld) {
  const int64_t row = (int64_t)blockIdx.x * kAleBlock + threadIdx.x;
  if (row >= n) return;
  const AleJob jb = load_job(jobs, blockIdx.y);
  const float x1 = X[row * ldx + jb.f1];
  int32_t cell = (x1 != x1) ? kAleNoCell : ale_interval(edges + jb.off1, jb.K1, x1) - 1;
  if (jb.f2 >= 0) {
    const float x2 = X[row * ldx + jb.f2];
    cell = (x1 != x1 || x2 != x2) ? kAleNoCell : cell * jb.K2 + ale_interval(edges + jb.off2, jb.K2, x2) - 1;
  }
  cells[(int64_t)blockIdx.y * ld + row] = cell;
}

// Rows [0, n) of one row chunk (blockIdx.x) for job blockIdx.y. X and out point at the chunk's first row;
// out[(job * C + c) * out_ld + row] = margin of corner c, C = 2 (1-D) or 4.
template <bool TWO>
__global__ __launch_bounds__(kAleBlock) void k_ale(const float* __restrict__ X, int64_t n, int F, int64_t ldx,
                                                   const uint2* __restrict__ nodes,
                                                   const int32_t* __restrict__ tree_ptr,
                                                   const int32_t* __restrict__ tile_ptr, int n_tiles,
                                                   float base_margin, const int32_t* __restrict__ jobs,
                                                   const float* __restrict__ edges, float* __restrict__ out,
                                                   int64_t out_ld, int tile_cap) {
  constexpr int C = TWO ? 4 : 2;
  const ForestBlock<kAleBlock> fb(tile_cap, F, n);
  const int64_t row = fb.row;
  const bool valid = row < n;
  fb.stage_rows<true>(X, F, ldx);
  const AleJob jb = load_job(jobs, blockIdx.y);  // block-uniform
  // the row's own interval edges, per lane; a row past n walks zeros, a NaN row the edges of interval 1
  GridVec<C> v1, v2, acc;
  {
    float lo1 = 0.0f, hi1 = 0.0f, lo2 = 0.0f, hi2 = 0.0f;
    if (valid) {
      const float* z1 = edges + jb.off1;
      const int k = ale_interval(z1, jb.K1, X[row * ldx + jb.f1]);
      lo1 = z1[k - 1];
      hi1 = z1[k];
      if constexpr (TWO) {
        const float* z2 = edges + jb.off2;
        const int l = ale_interval(z2, jb.K2, X[row * ldx + jb.f2]);
        lo2 = z2[l - 1];
        hi2 = z2[l];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      v1[c] = (c & 1) ? hi1 : lo1;
      v2[c] = (c & 2) ? hi2 : lo2;
      acc[c] = base_margin;
    }
  }
  const float* x = fb.x();
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    for (int t = t_begin; t < t_end; ++t) {
      const uint32_t base = (uint32_t)(tree_ptr[t] - nbase);
      walk_tree_points<0, C, C, TWO>(fb.s_nodes, base, fb.s_nodes[base], x, jb.f1, jb.f2, v1, v2, acc);
    }
  }
  if (valid) {
#pragma unroll
    for (int c = 0; c < C; ++c) out[((int64_t)blockIdx.y * C + c) * out_ld + row] = acc[c];
  }
}

// Block (cell, job): the entries [seg[cell], seg[cell + 1]) of the job's `order` row (chunk-local row indices
// of the rows in that cell, ascending) -> sums[(job * max_cells + cell) * 3 + 0..2] = (sum w d_margin,
// sum w d_prob, sum w). `corner`, `w` point at the chunk's first row. accumulate: add to the earlier chunks'.
// Entries outside [0, n) are skipped and segment bounds are clamped: nothing outside the chunk is read.
template <bool TWO>
__global__ __launch_bounds__(kAleBlock) void k_ale_reduce(const float* __restrict__ corner, int64_t corner_ld,
                                                          int64_t n, const float* __restrict__ w,
                                                          const int32_t* __restrict__ jobs,
                                                          const int32_t* __restrict__ order, int64_t order_ld,
                                                          const int32_t* __restrict__ seg_ptr, int max_cells,
                                                          double* __restrict__ sums, int accumulate) {
  constexpr int C = TWO ? 4 : 2;
  __shared__ double s[3][kAleBlock];
  const int cell = blockIdx.x, job = blockIdx.y, tid = threadIdx.x;
  const AleJob jb = load_job(jobs, job);
  if (cell >= jb.K1 * jb.K2) return;  // block-uniform
  const int32_t* seg = seg_ptr + (int64_t)job * (max_cells + 1);
  const int64_t b = min(max((int64_t)seg[cell], (int64_t)0), n);
  const int64_t e = min(max((int64_t)seg[cell + 1], b), n);
  const int32_t* ord = order + (int64_t)job * order_ld;
  const float* m0 = corner + (int64_t)job * C * corner_ld;
  double sm = 0.0, sp = 0.0, sw = 0.0;
  for (int64_t i = b + tid; i < e; i += kAleBlock) {
    const int64_t r = ord[i];
    if (r < 0 || r >= n) continue;
    const double wv = w ? (double)w[r] : 1.0;
    double m[C], p[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      m[c] = (double)m0[c * corner_ld + r];
      p[c] = 1.0 / (1.0 + exp(-m[c]));
    }
    double dm = m[1] - m[0], dp = p[1] - p[0];
    if constexpr (TWO) {
      dm = (m[3] - m[2]) - dm;
      dp = (p[3] - p[2]) - dp;
    }
    sm += wv * dm;
    sp += wv * dp;
    sw += wv;
  }
  s[0][tid] = sm;
  s[1][tid] = sp;
  s[2][tid] = sw;
  __syncthreads();
  for (int o = kAleBlock / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s[0][tid] += s[0][tid + o];
      s[1][tid] += s[1][tid + o];
      s[2][tid] += s[2][tid + o];
    }
    __syncthreads();
  }
  if (tid < 3) {
    double* dst = sums + ((int64_t)job * max_cells + cell) * 3 + tid;
    *dst = (accumulate ? *dst : 0.0) + s[tid][0];
  }
}

COBALT_API int64_t cobalt_ale_chunk_rows() { return kAleChunkRows; }
COBALT_API int cobalt_ale_max_intervals() { return kAleMaxIntervals; }
COBALT_API int cobalt_ale_max_cells() { return kAleMaxCells; }
COBALT_API int cobalt_ale_max_jobs() { return kAleMaxJobs; }
COBALT_API int cobalt_ale_no_cell() { return kAleNoCell; }

// Bytes of `workspace` for n rows, J jobs of `dims` (1 or 2) features: the corner margins of one row chunk,
// [J][C][min(n, chunk rows)] float32. Needed when sums are asked for without the per-row margins.
COBALT_API int64_t cobalt_ale_workspace(int64_t n, int J, int dims) {
  if (n <= 0 || J <= 0 || (dims != 1 && dims != 2)) return 0;
  return (int64_t)J * (dims == 2 ? 4 : 2) * std::min(n, kAleChunkRows) * (int64_t)sizeof(float);
}

// 0, or -8: J descriptors {f1, f2, off1, K1, off2, K2} of `dims` features each against F features and
// n_edges concatenated edges.
static int ale_check_jobs(const int32_t* jobs_host, int J, int dims, int F, int64_t n_edges) {
  if (jobs_host == nullptr || J < 1 || J > kAleMaxJobs || F < 1 || (dims != 1 && dims != 2)) return -8;
  for (int j = 0; j < J; ++j) {
    const int32_t* d = jobs_host + (int64_t)j * kAleJobInts;
    const int f1 = d[0], f2 = d[1], off1 = d[2], K1 = d[3], off2 = d[4], K2 = d[5];
    if (f1 < 0 || f1 >= F || K1 < 1 || K1 > kAleMaxIntervals || off1 < 0 || (int64_t)off1 + K1 + 1 > n_edges) return -8;
    if (dims == 1) {
      if (f2 != -1 || K2 != 1) return -8;
    } else {
      if (f2 < 0 || f2 >= F || f2 == f1 || K2 < 1 || K2 > kAleMaxIntervals || off2 < 0 ||
          (int64_t)off2 + K2 + 1 > n_edges || (int64_t)K1 * K2 > kAleMaxCells)
        return -8;
    }
  }
  return 0;
}

// cells: [J, n] int32 on the device, the input of the caller's per-chunk stable sort. Same refusals as
// cobalt_ale (-8); nothing is launched then.
COBALT_API int cobalt_ale_cells(const float* X, int64_t n, int F, int64_t ldx, const int32_t* jobs_host,
                                const int32_t* jobs, int J, int dims, const float* edges, int64_t n_edges,
                                int32_t* cells, hipStream_t stream) {
  if (const int rc = ale_check_jobs(jobs_host, J, dims, F, n_edges)) return rc;
  if (n < 0 || ldx < F || jobs == nullptr || edges == nullptr || cells == nullptr) return -8;
  if (n == 0) return 0;
  for (int64_t r0 = 0; r0 < n; r0 += kAleChunkRows) {
    const int64_t nc = std::min(kAleChunkRows, n - r0);
    hipLaunchKernelGGL(k_ale_cells, dim3(ceil_div(nc, kAleBlock), J), dim3(kAleBlock), 0, stream, X + r0 * ldx, nc,
                       ldx, jobs, edges, cells + r0, n);
    CK_LAUNCH();
  }
  return 0;
}

// jobs_host / jobs: the J descriptors on the host (checked here) and the same on the device (read by the
// kernels); dims = 1: every job is one feature (C = 2 corners), 2: a pair (C = 4). edges: n_edges float32 on
// the device, finite and strictly increasing per job and axis (the caller checks the contents).
// rows: [J, C, n] float32 corner margins or nullptr. sums: [J, max_cells, 3] doubles (sum w d_margin,
// sum w d_prob, sum w per cell; cells past a job's K1 * K2 are not written) or nullptr; they need `order`
// [J, n] int32 (per row chunk of cobalt_ale_chunk_rows() rows: the chunk-local indices of the chunk's rows
// sorted stably by cell) and seg_ptr [chunks, J, max_cells + 1] int32 (per chunk and job: the position in
// the chunk's order at which each cell starts; [max_cells] = the rows in any cell), and `workspace`
// (cobalt_ale_workspace) unless `rows` is given. Returns -2 / -3 for a tile or an LDS footprint outside the
// limits (as cobalt_pdp), -7 when sums are asked for without workspace (and without rows), -8 for a feature
// out of range, f1 == f2, an empty edge list, too many intervals or a missing argument; nothing is launched
// then.
COBALT_API int cobalt_ale(const float* X, int64_t n, int F, int64_t ldx, const void* nodes, const int32_t* tree_ptr,
                          const int32_t* tile_ptr, int n_tiles, int tile_cap, float base_margin,
                          const int32_t* jobs_host, const int32_t* jobs, int J, int dims, const float* edges,
                          int64_t n_edges, const float* w, const int32_t* order, const int32_t* seg_ptr,
                          int max_cells, float* rows, void* workspace, double* sums, hipStream_t stream) {
  if (const int rc = ale_check_jobs(jobs_host, J, dims, F, n_edges)) return rc;
  if (n < 0 || ldx < F || jobs == nullptr || edges == nullptr) return -8;
  const bool want_sums = sums != nullptr;
  if (want_sums) {
    if (order == nullptr || seg_ptr == nullptr || max_cells < 1 || max_cells > kAleMaxCells) return -8;
    for (int j = 0; j < J; ++j)
      if ((int64_t)jobs_host[j * kAleJobInts + 3] * jobs_host[j * kAleJobInts + 5] > max_cells) return -8;
  }
  if (const int rc = forest_limits(tile_cap, F, kAleBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kAleBlock);
  if (want_sums && rows == nullptr && workspace == nullptr) return -7;
  if (n == 0 || (rows == nullptr && !want_sums)) return 0;
  const bool two = dims == 2;
  const int C = two ? 4 : 2;
  const auto fn = two ? k_ale<true> : k_ale<false>;
  static size_t attr_set[2] = {kDefaultMaxLds, kDefaultMaxLds};
  CK(raise_dynamic_lds((const void*)fn, lds, attr_set[two ? 1 : 0]));
  const uint2* nd = static_cast<const uint2*>(nodes);
  const int64_t cap = std::min(n, kAleChunkRows);
  const dim3 block(kAleBlock);
  int chunk = 0;
  for (int64_t r0 = 0; r0 < n; r0 += kAleChunkRows, ++chunk) {
    const int64_t nc = std::min(kAleChunkRows, n - r0);
    float* out = rows ? rows + r0 : static_cast<float*>(workspace);
    const int64_t out_ld = rows ? n : cap;
    hipLaunchKernelGGL(fn, dim3(ceil_div(nc, kAleBlock), J), block, lds, stream, X + r0 * ldx, nc, F, ldx, nd,
                       tree_ptr, tile_ptr, n_tiles, base_margin, jobs, edges, out, out_ld, tile_cap);
    CK_LAUNCH();
    if (want_sums) {
      const int32_t* seg = seg_ptr + (int64_t)chunk * J * (max_cells + 1);
      hipLaunchKernelGGL(two ? k_ale_reduce<true> : k_ale_reduce<false>, dim3(max_cells, J), block, 0, stream, out,
                         out_ld, nc, w ? w + r0 : nullptr, jobs, order + r0, n, seg, max_cells, sums,
                         r0 > 0 ? 1 : 0);
      CK_LAUNCH();
    }
  }
  return 0;
}
