// Permutation feature importance of a tree ensemble (gfx950): job (i, r) scores every row n with x[feats[i]]
// replaced by cols[i][perm[r][n]] (the column's value of another row) and reduces the logloss / error terms
// of the job's margins; job 0, the baseline, substitutes nothing.
//
// A client of the packed-forest block of forest_walk.h (ForestBlock), like pdp.hip: one thread owns one row
// (features staged in LDS with the odd stride F | 1), tiles of the forest are staged in LDS, leaf values are
// added in fp32 in tree order starting from base_margin, so margins[job][n] has the bits of predict_margin on
// the substituted matrix. The substitution is the select of pdp_walk.h on the value read from LDS: neither X
// nor the staged row is written.
//
// Design choices
//  * blockIdx.y = 0 is the baseline, blockIdx.y = 1 + slot * ceil(R / kChunk) + c scores the repeats
//    [c * kChunk, + kChunk) of feature slot `slot`: a block stages its rows once and every forest tile once for
//    up to kChunk repeats, one fp32 accumulator per repeat. f1 = feats[slot] is block-uniform; the baseline
//    runs the same code with f1 = -1, which matches no node's 15-bit feature field. It is reduced in the same
//    order as every other job, so a feature that no tree splits on has importance exactly 0.0.
//  * The substituted values differ per lane: they are loaded before the tile loop into vector registers,
//    cols[slot][perm[r][row]] -- perm is read coalesced, the gather goes to the contiguous 4 N-byte column
//    (never to row-major X). perm entries are global row indices: the row chunks below offset perm, y, w and
//    the outputs, not cols.
//  * Only the chunk's live repeats are walked: whole groups of kWalk chains (pdp_walk.h walk_tree_points)
//    and one shorter group for the remainder (R = 5: 4 + 1 chains, the baseline: 1 chain). Accumulators past
//    the live repeats keep base_margin and are never written. `live` is block-uniform.
//  * No "tree does not use f1" shortcut: it was not measured, so it is not there.
//  * Sums: per job sum w loss and sum w err with, in fp64 from the fp32 margin m, loss = log1p(exp(-|m|)) +
//    max(m, 0) - y m and err = (m > 0) != (y > 0.5) (wave_partials.h, as evalcurve.hip); the 64 lanes of a wave
//    are summed by a fixed DPP sequence, the wave's pair goes to workspace[job][wave], and k_pair_reduce adds a
//    job's partials in a fixed order. No floating-point atomics: the same input gives the same bits on every
//    run. Rows past n in the last block walk a row of zeros with weight 0.0 and take part in every wave sum.
//  * Rows are processed in chunks of kPermChunkRows = 2^17 (2048 wave partials per job: 32 KiB of workspace
//    per job); chunk sums are added in chunk order.
#include "common.h"
#include "pdp_walk.h"
#include "wave_partials.h"
#include <algorithm>

using namespace cobalt;

namespace {
constexpr int kPermBlock = 256;
constexpr int kPermRepChunk = 16;    // default repeats per block (8 is also built; measured in docs/PERF.md)
constexpr int64_t kPermChunkRows = 1 << 17;
constexpr int kPermMaxJobs = 1 << 20;

// One tree for the repeats [0, live) of the chunk: groups of kWalk chains, then one group of live % kWalk.
// `live` is the same in every lane of the block.
template <int kChunk, int J = 0>
__device__ __forceinline__ void walk_tree_live(const uint2* s_nodes, uint32_t base, const float* x, int f1, int live,
                                               const GridVec<kChunk> v, GridVec<kChunk>& acc) {
  if constexpr (J < kChunk) {
    const int left = live - J;
    if (left >= kWalk) {
      walk_tree_points<J, kChunk, kWalk, false>(s_nodes, base, s_nodes[base], x, f1, -1, v, v, acc);
      walk_tree_live<kChunk, J + kWalk>(s_nodes, base, x, f1, live, v, acc);
    } else if (left == 3) {
      walk_tree_points<J, kChunk, 3, false>(s_nodes, base, s_nodes[base], x, f1, -1, v, v, acc);
    } else if (left == 2) {
      walk_tree_points<J, kChunk, 2, false>(s_nodes, base, s_nodes[base], x, f1, -1, v, v, acc);
    } else if (left == 1) {
      walk_tree_points<J, kChunk, 1, false>(s_nodes, base, s_nodes[base], x, f1, -1, v, v, acc);
    }
  }
}
}  // namespace

// Rows [0, n) of one row chunk (blockIdx.x). X, perm, y, w and margins point at the chunk's first row; cols
// does not (perm holds global row indices). perm: [R, ldn], cols: [nf, ldn], margins: [1 + nf R, ldn].
// SUMS: every wave writes part[job][wave] = (sum w loss, sum w err) (rows of `nparts` pairs) and the waves of
// the baseline block write wpart[wave] = sum w.
template <bool SUMS, int kChunk>
__global__ __launch_bounds__(kPermBlock) void k_permimp(
    const float* __restrict__ X, int64_t n, int F, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ w, const uint2* __restrict__ nodes, const int32_t* __restrict__ tree_ptr,
    const int32_t* __restrict__ tile_ptr, int n_tiles, float base_margin, const int32_t* __restrict__ feats,
    const float* __restrict__ cols, const int32_t* __restrict__ perm, int R, int64_t ldn,
    float* __restrict__ margins, double* __restrict__ part, double* __restrict__ wpart, int nparts, int tile_cap) {
  const ForestBlock<kPermBlock> fb(tile_cap, F, n);
  const int64_t row = fb.row;
  const bool valid = row < n;
  fb.stage_rows<true>(X, F, ldx);
  // the block's jobs (block-uniform): the baseline, or `live` repeats of one feature slot from repeat k0 on
  const int rep_chunks = (R + kChunk - 1) / kChunk;
  int f1 = -1, k0 = 0, live = 1, job0 = 0;
  if (blockIdx.y > 0) {
    const int slot = ((int)blockIdx.y - 1) / rep_chunks;
    k0 = (((int)blockIdx.y - 1) - slot * rep_chunks) * kChunk;
    live = min(kChunk, R - k0);
    f1 = feats[slot];
    job0 = 1 + slot * R + k0;
    cols += (int64_t)slot * ldn;
  }
  GridVec<kChunk> v, acc;
#pragma unroll
  for (int j = 0; j < kChunk; ++j) {
    float a = 0.0f;
    if (blockIdx.y > 0 && j < live && valid) a = cols[perm[(int64_t)(k0 + j) * ldn + row]];
    v[j] = a;
    acc[j] = base_margin;
  }
  const float* x = fb.x();
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int t_begin = tile_ptr[tile], t_end = tile_ptr[tile + 1];
    const int nbase = fb.stage_tile(nodes, tree_ptr, t_begin, t_end);
    for (int t = t_begin; t < t_end; ++t)
      walk_tree_live<kChunk>(fb.s_nodes, (uint32_t)(tree_ptr[t] - nbase), x, f1, live, v, acc);
  }
  if (margins && valid) {
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (j < live) margins[(int64_t)(job0 + j) * ldn + row] = acc[j];
  }
  if constexpr (SUMS) {
    const int wave_g = blockIdx.x * (kPermBlock / kWave) + wave_id();  // < nparts
    double yv = 0.0, wv = 0.0;
    bool ypos = false;
    if (valid) {
      const float yf = y[row];
      yv = (double)yf;
      ypos = yf > 0.5f;
      wv = w ? (double)w[row] : 1.0;
    }
    if (blockIdx.y == 0) {
      const double sw = wave_total_f64(wv);
      if (lane_id() == kWave - 1) wpart[wave_g] = sw;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
      if (j < live) {
        const double m = (double)acc[j];
        const double loss = logloss_term(m, yv);
        const double err = error_term(acc[j], ypos);
        const double sl = wave_total_f64(valid ? wv * loss : 0.0);
        const double se = wave_total_f64(valid ? wv * err : 0.0);
        if (lane_id() == kWave - 1) {
          double* dst = part + ((int64_t)(job0 + j) * nparts + wave_g) * 2;
          dst[0] = sl;
          dst[1] = se;
        }
      }
    }
  }
}

static int64_t perm_parts(int64_t n) { return wave_parts(n, kPermChunkRows, kPermBlock); }

COBALT_API int cobalt_perm_rep_chunk() { return kPermRepChunk; }
COBALT_API int64_t cobalt_perm_chunk_rows() { return kPermChunkRows; }

// Bytes of `workspace` for n rows and `jobs` = 1 + nf * R jobs: [jobs][parts][2] + [parts] doubles with
// parts = the waves of one row chunk.
COBALT_API int64_t cobalt_perm_workspace(int64_t n, int jobs) {
  if (n <= 0 || jobs <= 0) return 0;
  return wave_partials_bytes(jobs, perm_parts(n));
}

// Jobs: 0 = the baseline, 1 + i * R + r = feature slot i under perm[r]. feats: nf int32 ON THE DEVICE, each in
// [0, F); cols: [nf, n] float32, cols[i][m] = X[m][feats[i]]; perm: [R, n] int32, every entry in [0, n) (the
// caller checks the contents of feats and perm: the kernel reads cols[i][perm[r][m]] unchecked).
// margins: [1 + nf R, n] float32 or nullptr; sums: [2 (1 + nf R) + 1] doubles ((sum w loss, sum w err) per
// job, then sum w) or nullptr (y, w and workspace are not touched then). rep_chunk: repeats per block, 8 or
// 16, 0 = cobalt_perm_rep_chunk(). Returns -2 / -3 for a tile or an LDS footprint outside the limits (as
// cobalt_pdp), -7 when sums are asked for without workspace, -8 for arguments outside their ranges; nothing
// is launched then.
COBALT_API int cobalt_perm_importance(const float* X, int64_t n, int F, int64_t ldx, const void* nodes,
                                      const int32_t* tree_ptr, const int32_t* tile_ptr, int n_tiles, int tile_cap,
                                      float base_margin, const int32_t* feats, int nf, const float* cols,
                                      const int32_t* perm, int R, const float* y, const float* w, float* margins,
                                      void* workspace, double* sums, int rep_chunk, hipStream_t stream) {
  if (rep_chunk == 0) rep_chunk = kPermRepChunk;
  if (F < 1 || nf < 0 || n < 0 || ldx < F || (rep_chunk != 8 && rep_chunk != 16)) return -8;
  if (nf > 0 && (R < 1 || feats == nullptr || cols == nullptr || perm == nullptr)) return -8;
  if (nf == 0) R = 1;
  if ((int64_t)nf * R + 1 > kPermMaxJobs || (int64_t)nf * ceil_div(R, rep_chunk) + 1 > 65535) return -8;
  const bool want_sums = sums != nullptr;
  if (want_sums && y == nullptr) return -8;
  if (const int rc = forest_limits(tile_cap, F, kPermBlock)) return rc;
  const size_t lds = forest_lds_bytes(tile_cap, F, kPermBlock);
  if (want_sums && workspace == nullptr) return -7;
  if (n == 0 || (margins == nullptr && !want_sums)) return 0;
  using Kernel = decltype(&k_permimp<false, 8>);
  static const Kernel kernels[4] = {k_permimp<false, 8>, k_permimp<false, 16>, k_permimp<true, 8>,
                                    k_permimp<true, 16>};
  const int which = (want_sums ? 2 : 0) + (rep_chunk == 16 ? 1 : 0);
  const Kernel fn = kernels[which];
  static size_t attr_set[4] = {kDefaultMaxLds, kDefaultMaxLds, kDefaultMaxLds, kDefaultMaxLds};
  CK(raise_dynamic_lds((const void*)fn, lds, attr_set[which]));
  const uint2* nd = static_cast<const uint2*>(nodes);
  const int J = 1 + nf * R;
  const int nparts = (int)perm_parts(n);
  double* part = want_sums ? static_cast<double*>(workspace) : nullptr;
  double* wpart = wave_wpart(part, J, nparts);
  const dim3 block(kPermBlock);
  for (int64_t r0 = 0; r0 < n; r0 += kPermChunkRows) {
    const int64_t nc = std::min(kPermChunkRows, n - r0);
    const dim3 grid(ceil_div(nc, kPermBlock), 1 + nf * ceil_div(R, rep_chunk));
    hipLaunchKernelGGL(fn, grid, block, lds, stream, X + r0 * ldx, nc, F, ldx, want_sums ? y + r0 : nullptr,
                       (want_sums && w) ? w + r0 : nullptr, nd, tree_ptr, tile_ptr, n_tiles, base_margin, feats, cols,
                       perm ? perm + r0 : nullptr, R, n, margins ? margins + r0 : nullptr, part, wpart, nparts,
                       tile_cap);
    CK_LAUNCH();
    if (want_sums) {
      hipLaunchKernelGGL(k_pair_reduce<>, dim3(J + 1), dim3(kReduceBlock), 0, stream, part, wpart, nparts,
                         (int)perm_parts(nc), J, sums, r0 > 0 ? 1 : 0);
      CK_LAUNCH();
    }
  }
  return 0;
}
