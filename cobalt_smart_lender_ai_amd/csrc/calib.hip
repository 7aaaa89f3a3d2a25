// Score calibration on the device (gfx950): the isotonic fit's convex hull, the piecewise-linear apply and the
// reliability table. The definitions are in metrics/calibration.py (iso_hull_host, calib_apply_host,
// reliability_sums_host); iso_hull_tiled_host is this file's hull decomposition on the host. The hull and the
// table are exact integers and the apply is a fixed sequence of fp64 operations, so host and device give the
// same bits.
//
// cobalt_iso_hull. Input: cw, cs int64 [m] (m = groups + 1), cw strictly increasing from 0, cs non-decreasing
// from 0, both at most 2^31 - 1, so they are staged as 32-bit words and every product of two differences fits
// int64. Output: the indices of the strict lower convex hull, ascending, and their number. Vertex b (above a) is
// popped under k when (cs[b]-cs[a]) (cw[k]-cw[b]) >= (cs[k]-cs[b]) (cw[b]-cw[a]).
//  * A vertex of the whole hull is a vertex of the hull of any contiguous tile that holds it, so the hull of the
//    union of tile hulls is the hull. k_iso_tiles: one block per kIsoTileRows consecutive survivors, staged in
//    LDS (24 KiB). Every point starts as a run of one; runs are merged pairwise in log steps, one thread per
//    merge. A run's hull is a doubly linked list through LDS (its first and last point are always on it), so a
//    merge moves nothing: it pushes the right run's points onto the left run's stack, popping through the
//    `prv` links, and stops at the first push after the right run's first that pops nothing; from there the
//    right hull's own links are already right. A popped point is never on a later hull: its `alive` byte is
//    cleared, and a block-wide scan of those bytes writes the tile's hull in index order.
//  * A round is k_iso_tiles (hulls into tile-strided slots), k_iso_scan (one block: exclusive prefix of the
//    tiles' counts, the round's survivor count) and k_iso_gather (slots to a dense list). m <= kIsoTileRows
//    takes no round; anything larger takes kIsoRounds = 2, whatever the tiles shed. The later round's and the
//    last stage's sizes are device counts: grids are sized for no shedding at all and surplus blocks exit.
//  * k_iso_final: one block. Up to kIsoTileRows survivors are one more tile; more (an input whose tiles shed
//    next to nothing) are chained by one thread from global memory: slow, bounded by the survivor count, right.
//  * No atomics; the only thing the host reads is the final count.
//
// cobalt_calib_apply. out[i] = vk[j] + (vk[j+1]-vk[j]) * ((double)x - xk[j]) / ((double)xk[j+1] - xk[j]) with x
// clipped to [xk[0], xk[K-1]] and xk[j] <= x < xk[j+1] (j = K - 2 at the top), rounded to float32; K = 1 gives
// vk[0]; NaN gives the quiet NaN 0x7fc00000. Contraction is off: an FMA would round differently from the host.
// Up to kCalibLdsKnots = 4096 knots are staged in LDS (12 bytes each, 48 KiB); above that the search reads
// global memory. The search is a branch-free lower bound with a uniform trip count; rows are loaded and stored
// 16 bytes a lane when x and out are 16-byte aligned.
//
// cobalt_reliability_sums. out int64 [3, B] += (W, S, Pq) per bin, bin = #{interior edges <= p}, Pq = sum wq *
// rint(p * 2^30). Up to kRelLdsBins = 2048 bins: per-block LDS counters (W, S 32-bit, Pq 64-bit) and the edges in
// LDS (40 KiB at most), flushed with 64-bit global atomics; integers commute, so the table does not depend on
// the order. A weight is at most 2^20 and a tile has 2048 rows, so a 32-bit counter holds a tile: with weights
// the block flushes after every tile, without it flushes once (at most 2^28 rows of weight 1). Above 2048 bins
// (to kRelMaxBins = 4096) the counters would not fit beside the edges: rows add to the table directly.
//
// Refusals come before any launch.
//  cobalt_iso_hull: -1 m < 2, -2 m > 2^28 + 1, -3 total weight < 1 or > 2^31 - 1, -4 a pointer missing,
//    -5 workspace too small.
//  cobalt_calib_apply: -1 n < 0, -2 K < 1, -3 a pointer missing.
//  cobalt_reliability_sums: -1 n < 0, -2 B < 1 or B > 4096, -3 p, y or out missing, -4 edges missing with B > 1.
#include "common.h"
#include <algorithm>
#include <limits.h>

using namespace cobalt;

namespace {
constexpr int kIsoTileRows = 2048;
constexpr int kIsoBlock = 256;
constexpr int kIsoPerThread = kIsoTileRows / kIsoBlock;
constexpr int kIsoScanBlock = 1024;
constexpr int kIsoRounds = 2;
constexpr int64_t kIsoMaxPoints = ((int64_t)1 << 28) + 1;
constexpr int64_t kIsoMaxWeight = 2147483647;
static_assert(kIsoTileRows <= 65536, "the links are 16-bit");
static_assert(kIsoTileRows % kIsoBlock == 0, "a thread compacts a whole number of slots");

constexpr int kCalibLdsKnots = 4096;
constexpr int kCalibBlock = 256;
constexpr int kCalibMaxBlocks = 2048;

constexpr int kRelBlock = 256;
constexpr int kRelTileRows = 2048;
constexpr int kRelLdsBins = 2048;
constexpr int kRelMaxBins = 4096;
constexpr int kRelMaxBlocks = 1024;
constexpr double kRelPScale = 1073741824.0;  // 2^30
static_assert((int64_t)kRelTileRows << 20 < ((int64_t)1 << 32), "a tile of maximum weights must fit a counter");

struct IsoTile {
  uint32_t w[kIsoTileRows];
  uint32_t s[kIsoTileRows];
  uint16_t nxt[kIsoTileRows];
  uint16_t prv[kIsoTileRows];
  uint8_t alive[kIsoTileRows];
  int wave_tot[kIsoBlock / kWave];
};

// slope(a, b) >= slope(b, k): b is not a vertex of the strict lower hull once k is there.
__device__ __forceinline__ bool iso_pop(uint32_t wa, uint32_t sa, uint32_t wb, uint32_t sb, uint32_t wk, uint32_t sk) {
  return (int64_t)(sb - sa) * (int64_t)(wk - wb) >= (int64_t)(sk - sb) * (int64_t)(wb - wa);
}

// The hull of the n <= kIsoTileRows survivors [base0, base0 + n) of `in` (null: survivor q is point q), written
// in index order to out[0 ..); returns their number (block-uniform). All kIsoBlock threads must call it.
__device__ int iso_tile_hull(IsoTile& t, const int64_t* __restrict__ cw, const int64_t* __restrict__ cs,
                             const int32_t* __restrict__ in, int64_t base0, int n, int32_t* __restrict__ out) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += kIsoBlock) {
    const int64_t g = in ? (int64_t)in[base0 + i] : base0 + i;
    t.w[i] = (uint32_t)cw[g];
    t.s[i] = (uint32_t)cs[g];
    t.alive[i] = 1;
  }
  __syncthreads();
  for (int h = 1; h < n; h <<= 1) {
    const int pairs = (n + 2 * h - 1) / (2 * h);
    for (int p = tid; p < pairs; p += kIsoBlock) {
      const int a = p * 2 * h, m = a + h;
      if (m >= n) continue;
      const int b = min(a + 2 * h, n);
      int top = m - 1, r = m, j = 0;
      while (true) {
        const int rn = (r == b - 1) ? -1 : (int)t.nxt[r];
        const uint32_t wr = t.w[r], sr = t.s[r];
        uint32_t wt = t.w[top], st = t.s[top];
        bool popped = false;
        while (top != a) {
          const int q = (int)t.prv[top];
          const uint32_t wq = t.w[q], sq = t.s[q];
          if (!iso_pop(wq, sq, wt, st, wr, sr)) break;
          t.alive[top] = 0;
          top = q;
          wt = wq;
          st = sq;
          popped = true;
        }
        t.nxt[top] = (uint16_t)r;
        t.prv[r] = (uint16_t)top;
        if (rn < 0 || (!popped && j >= 1)) break;
        top = r;
        r = rn;
        ++j;
      }
    }
    __syncthreads();
  }
  // ordered compaction: a thread owns kIsoPerThread consecutive slots
  const int i0 = tid * kIsoPerThread;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kIsoPerThread; ++k) mine += (i0 + k < n && t.alive[i0 + k]) ? 1 : 0;
  const int incl = wave_incl_scan(mine);
  if (lane_id() == kWave - 1) t.wave_tot[wave_id()] = incl;
  __syncthreads();
  int before = incl - mine, total = 0;
#pragma unroll
  for (int v = 0; v < kIsoBlock / kWave; ++v) {
    const int c = t.wave_tot[v];
    before += v < wave_id() ? c : 0;
    total += c;
  }
#pragma unroll
  for (int k = 0; k < kIsoPerThread; ++k) {
    const int i = i0 + k;
    if (i < n && t.alive[i]) out[before++] = in ? in[base0 + i] : (int32_t)(base0 + i);
  }
  return total;
}
}  // namespace

// Block t: the hull of survivors [t T, (t + 1) T) into slots[t T ..) and its size into tile_cnt[t]. The survivor
// count is *cnt_in (a device count of the round before) or n_host.
__global__ __launch_bounds__(kIsoBlock) void k_iso_tiles(const int64_t* __restrict__ cw, const int64_t* __restrict__ cs,
                                                         const int32_t* __restrict__ in, int64_t n_host,
                                                         const int32_t* __restrict__ cnt_in,
                                                         int32_t* __restrict__ slots, int32_t* __restrict__ tile_cnt) {
  __shared__ IsoTile t;
  const int64_t cnt = cnt_in ? (int64_t)*cnt_in : n_host;
  const int64_t base0 = (int64_t)blockIdx.x * kIsoTileRows;
  if (base0 >= cnt) return;
  const int n = (int)min((int64_t)kIsoTileRows, cnt - base0);
  const int total = iso_tile_hull(t, cw, cs, in, base0, n, slots + base0);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// One block: tile_off[t] = sum of tile_cnt[0 .. t) over the live tiles, *cnt_out = their sum.
__global__ __launch_bounds__(kIsoScanBlock) void k_iso_scan(const int32_t* __restrict__ tile_cnt, int64_t n_host,
                                                            const int32_t* __restrict__ cnt_in,
                                                            int32_t* __restrict__ tile_off,
                                                            int32_t* __restrict__ cnt_out) {
  __shared__ int s_tot[kIsoScanBlock / kWave];
  const int tid = threadIdx.x;
  const int64_t cnt = cnt_in ? (int64_t)*cnt_in : n_host;
  const int nt = (int)((cnt + kIsoTileRows - 1) / kIsoTileRows);
  const int per = (nt + kIsoScanBlock - 1) / kIsoScanBlock;
  const int lo = min(tid * per, nt), hi = min(lo + per, nt);
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += tile_cnt[i];
  const int incl = wave_incl_scan(mine);
  if (lane_id() == kWave - 1) s_tot[wave_id()] = incl;
  __syncthreads();
  int run = incl - mine, total = 0;
#pragma unroll
  for (int v = 0; v < kIsoScanBlock / kWave; ++v) {
    const int c = s_tot[v];
    run += v < wave_id() ? c : 0;
    total += c;
  }
  for (int i = lo; i < hi; ++i) {
    tile_off[i] = run;
    run += tile_cnt[i];
  }
  if (tid == 0) *cnt_out = total;
}

// Block t: its tile's hull from slots[t T ..) to dense[tile_off[t] ..).
__global__ __launch_bounds__(kIsoBlock) void k_iso_gather(const int32_t* __restrict__ slots,
                                                          const int32_t* __restrict__ tile_cnt,
                                                          const int32_t* __restrict__ tile_off, int64_t n_host,
                                                          const int32_t* __restrict__ cnt_in,
                                                          int32_t* __restrict__ dense) {
  const int64_t cnt = cnt_in ? (int64_t)*cnt_in : n_host;
  const int64_t base0 = (int64_t)blockIdx.x * kIsoTileRows;
  if (base0 >= cnt) return;
  const int c = tile_cnt[blockIdx.x];
  const int64_t o = tile_off[blockIdx.x];
  for (int i = threadIdx.x; i < c; i += kIsoBlock) dense[o + i] = slots[base0 + i];
}

// One block: the hull of whatever is left, into out / *out_cnt.
__global__ __launch_bounds__(kIsoBlock) void k_iso_final(const int64_t* __restrict__ cw, const int64_t* __restrict__ cs,
                                                         const int32_t* __restrict__ in, int64_t n_host,
                                                         const int32_t* __restrict__ cnt_in, int32_t* __restrict__ out,
                                                         int32_t* __restrict__ out_cnt) {
  __shared__ IsoTile t;
  const int64_t cnt = cnt_in ? (int64_t)*cnt_in : n_host;
  if (cnt <= kIsoTileRows) {
    const int total = iso_tile_hull(t, cw, cs, in, 0, (int)cnt, out);
    if (threadIdx.x == 0) *out_cnt = total;
    return;
  }
  if (threadIdx.x != 0) return;
  int64_t sp = 0;
  uint32_t wa = 0, sa = 0, wb = 0, sb = 0;  // the two points on top of the stack: a below b
  for (int64_t k = 0; k < cnt; ++k) {
    const int32_t id = in ? in[k] : (int32_t)k;
    const uint32_t wk = (uint32_t)cw[id], sk = (uint32_t)cs[id];
    while (sp >= 2 && iso_pop(wa, sa, wb, sb, wk, sk)) {
      --sp;
      wb = wa;
      sb = sa;
      if (sp >= 2) {
        const int32_t ia = out[sp - 2];
        wa = (uint32_t)cw[ia];
        sa = (uint32_t)cs[ia];
      }
    }
    out[sp++] = id;
    wa = wb;
    sa = sb;
    wb = wk;
    sb = sk;
  }
  *out_cnt = (int32_t)sp;
}

// ------------------------------------------------------------------------------------------------- apply
namespace {
__device__ __forceinline__ float calib_eval(float x, const float* kx, const double* kv, int K) {
#pragma clang fp contract(off)
  const float qnan = __int_as_float(0x7fc00000);
  if (K == 1) return x != x ? qnan : (float)kv[0];
  const float xc = fminf(fmaxf(x, kx[0]), kx[K - 1]);  // a NaN x becomes kx[0] here and NaN again below
  int lo = 0, len = K;
  while (len > 1) {  // the last knot <= xc; kx[0] <= xc holds
    const int half = len >> 1;
    lo = kx[lo + half] <= xc ? lo + half : lo;
    len -= half;
  }
  const int j = min(lo, K - 2);
  const double x0 = (double)kx[j], x1 = (double)kx[j + 1], v0 = kv[j], v1 = kv[j + 1];
  const double d = v1 - v0;
  const double u = (double)xc - x0;
  const double prod = d * u;
  const double quot = prod / (x1 - x0);
  const double r = v0 + quot;
  return x != x ? qnan : (float)r;
}
}  // namespace

template <bool LDS, bool VEC>
__global__ __launch_bounds__(kCalibBlock) void k_calib_apply(const float* __restrict__ x, int64_t n,
                                                             const float* __restrict__ xk,
                                                             const double* __restrict__ vk, int K,
                                                             float* __restrict__ out) {
  extern __shared__ unsigned long long s_dyn[];
  const float* kx = xk;
  const double* kv = vk;
  if constexpr (LDS) {
    double* sv = reinterpret_cast<double*>(s_dyn);  // [K] values, then [K] positions
    float* sx = reinterpret_cast<float*>(sv + K);
    for (int i = threadIdx.x; i < K; i += kCalibBlock) {
      sv[i] = vk[i];
      sx[i] = xk[i];
    }
    __syncthreads();
    kx = sx;
    kv = sv;
  }
  const int64_t gtid = (int64_t)blockIdx.x * kCalibBlock + threadIdx.x;
  const int64_t gsz = (int64_t)gridDim.x * kCalibBlock;
  if constexpr (VEC) {
    const int64_t n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int64_t i = gtid; i < n4; i += gsz) {
      const float4 v = x4[i];
      float4 r;
      r.x = calib_eval(v.x, kx, kv, K);
      r.y = calib_eval(v.y, kx, kv, K);
      r.z = calib_eval(v.z, kx, kv, K);
      r.w = calib_eval(v.w, kx, kv, K);
      o4[i] = r;
    }
    const int64_t i = (n4 << 2) + gtid;  // the last n % 4 rows
    if (i < n) out[i] = calib_eval(x[i], kx, kv, K);
  } else {
    for (int64_t i = gtid; i < n; i += gsz) out[i] = calib_eval(x[i], kx, kv, K);
  }
}

// ------------------------------------------------------------------------------------------- reliability
namespace {
// #{i : e[i] <= x} over e[0 .. E): searchsorted "right".
__device__ __forceinline__ int edges_le(const float* e, int E, float x) {
  int lo = 0, hi = E;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
}  // namespace

// Block x: the tiles [x tiles_per_block, (x + 1) tiles_per_block) of the rows. out: [3, B] (W, S, Pq), added to.
template <bool HAS_W, bool LDSC>
__global__ __launch_bounds__(kRelBlock) void k_rel_sums(const float* __restrict__ p, const float* __restrict__ y,
                                                        const int32_t* __restrict__ wq, int64_t n,
                                                        const float* __restrict__ edges, int B,
                                                        unsigned long long* __restrict__ out, int tiles_per_block) {
  extern __shared__ unsigned long long s_dyn[];
  const int tid = threadIdx.x;
  const int E = B - 1;
  unsigned long long* s_pq = s_dyn;                               // [B]
  uint32_t* s_w = reinterpret_cast<uint32_t*>(s_dyn + (LDSC ? B : 0));  // [B]
  uint32_t* s_s = s_w + (LDSC ? B : 0);                           // [B]
  float* s_e = reinterpret_cast<float*>(s_s + (LDSC ? B : 0));    // [E]
  const float* e = edges;
  if constexpr (LDSC) {
    for (int i = tid; i < B; i += kRelBlock) {
      s_pq[i] = 0ull;
      s_w[i] = 0u;
      s_s[i] = 0u;
    }
    for (int i = tid; i < E; i += kRelBlock) s_e[i] = edges[i];
    __syncthreads();
    e = s_e;
  }
  const int64_t ntiles = (n + kRelTileRows - 1) / kRelTileRows;
  const int64_t t_begin = (int64_t)blockIdx.x * tiles_per_block;
  const int64_t t_end = min(t_begin + tiles_per_block, ntiles);
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t r0 = t * kRelTileRows;
    const int rows = (int)min((int64_t)kRelTileRows, n - r0);
    for (int r = tid; r < rows; r += kRelBlock) {
      const float pv = p[r0 + r];
      const bool pos = y[r0 + r] > 0.5f;
      uint32_t w = 1u;
      if constexpr (HAS_W) w = (uint32_t)wq[r0 + r];
      const int b = edges_le(e, E, pv);
      const unsigned long long q = (unsigned long long)__double2ll_rn((double)pv * kRelPScale);
      if (w != 0u) {
        if constexpr (LDSC) {
          atomicAdd(&s_w[b], w);
          if (pos) atomicAdd(&s_s[b], w);
          atomicAdd(&s_pq[b], (unsigned long long)w * q);
        } else {
          atomicAdd(&out[b], (unsigned long long)w);
          if (pos) atomicAdd(&out[B + b], (unsigned long long)w);
          atomicAdd(&out[2 * (int64_t)B + b], (unsigned long long)w * q);
        }
      }
    }
    if constexpr (LDSC) {
      if (HAS_W || t + 1 == t_end) {
        __syncthreads();
        for (int i = tid; i < B; i += kRelBlock) {
          const uint32_t cw_ = s_w[i];
          if (cw_ != 0u) {
            atomicAdd(&out[i], (unsigned long long)cw_);
            const uint32_t cs_ = s_s[i];
            if (cs_ != 0u) atomicAdd(&out[B + i], (unsigned long long)cs_);
            const unsigned long long cq = s_pq[i];
            if (cq != 0ull) atomicAdd(&out[2 * (int64_t)B + i], cq);
            s_w[i] = 0u;
            s_s[i] = 0u;
            s_pq[i] = 0ull;
          }
        }
        __syncthreads();
      }
    }
  }
}

COBALT_API int cobalt_iso_tile_rows() { return kIsoTileRows; }
COBALT_API int cobalt_iso_rounds() { return kIsoRounds; }
COBALT_API int cobalt_calib_lds_knots() { return kCalibLdsKnots; }
COBALT_API int cobalt_reliability_lds_bins() { return kRelLdsBins; }
COBALT_API int cobalt_reliability_max_bins() { return kRelMaxBins; }

// Bytes of workspace for m points (two index lists, the tiles' counts and offsets, the rounds' counts), or the
// refusal of cobalt_iso_hull for this m.
COBALT_API int64_t cobalt_iso_hull_workspace_bytes(int64_t m) {
  if (m < 2) return -1;
  if (m > kIsoMaxPoints) return -2;
  if (m <= kIsoTileRows) return 8;
  const int64_t nt = (m + kIsoTileRows - 1) / kIsoTileRows;
  return (2 * m + 2 * nt + kIsoRounds + 1) / 2 * 8 + 8;
}

// cw, cs: int64 [m] on the device (layout above); total_weight = cw[m - 1], which the caller knows. out_idx:
// int32 [m], out_cnt: int32 [1], both on the device; the hull's indices are out_idx[0 .. *out_cnt) once the
// stream has run. rounds_cnt, when given, is a device int32 [kIsoRounds] that receives the survivor count of
// every round (untouched when m fits one tile).
COBALT_API int cobalt_iso_hull(const int64_t* cw, const int64_t* cs, int64_t m, int64_t total_weight,
                               void* workspace, int64_t workspace_bytes, int32_t* out_idx, int32_t* out_cnt,
                               int32_t* rounds_cnt, hipStream_t stream) {
  const int64_t need = cobalt_iso_hull_workspace_bytes(m);
  if (need < 0) return (int)need;
  if (total_weight < 1 || total_weight > kIsoMaxWeight) return -3;
  if (cw == nullptr || cs == nullptr || out_idx == nullptr || out_cnt == nullptr) return -4;
  if (m > kIsoTileRows && (workspace == nullptr || workspace_bytes < need)) return (workspace == nullptr) ? -4 : -5;
  if (m <= kIsoTileRows) {
    hipLaunchKernelGGL(k_iso_final, dim3(1), dim3(kIsoBlock), 0, stream, cw, cs, (const int32_t*)nullptr, m,
                       (const int32_t*)nullptr, out_idx, out_cnt);
    CK_LAUNCH();
    return 0;
  }
  const int64_t nt = (m + kIsoTileRows - 1) / kIsoTileRows;
  int32_t* slots = static_cast<int32_t*>(workspace);
  int32_t* dense = slots + m;
  int32_t* tile_cnt = dense + m;
  int32_t* tile_off = tile_cnt + nt;
  int32_t* counts = tile_off + nt;  // [kIsoRounds]
  const int32_t* in = nullptr;
  const int32_t* cnt_in = nullptr;
  for (int r = 0; r < kIsoRounds; ++r) {
    hipLaunchKernelGGL(k_iso_tiles, dim3((unsigned)nt), dim3(kIsoBlock), 0, stream, cw, cs, in, m, cnt_in, slots,
                       tile_cnt);
    CK_LAUNCH();
    hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(kIsoScanBlock), 0, stream, (const int32_t*)tile_cnt, m, cnt_in,
                       tile_off, counts + r);
    CK_LAUNCH();
    hipLaunchKernelGGL(k_iso_gather, dim3((unsigned)nt), dim3(kIsoBlock), 0, stream, (const int32_t*)slots,
                       (const int32_t*)tile_cnt, (const int32_t*)tile_off, m, cnt_in, dense);
    CK_LAUNCH();
    in = dense;
    cnt_in = counts + r;
  }
  hipLaunchKernelGGL(k_iso_final, dim3(1), dim3(kIsoBlock), 0, stream, cw, cs, in, m, cnt_in, out_idx, out_cnt);
  CK_LAUNCH();
  if (rounds_cnt != nullptr)
    CK(hipMemcpyAsync(rounds_cnt, counts, kIsoRounds * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  return 0;
}

// x: float32 [n], xk: float32 [K] strictly increasing, vk: float64 [K], out: float32 [n], all on the device.
COBALT_API int cobalt_calib_apply(const float* x, int64_t n, const float* xk, const double* vk, int K, float* out,
                                  hipStream_t stream) {
  if (n < 0) return -1;
  if (K < 1) return -2;
  if (xk == nullptr || vk == nullptr || (n > 0 && (x == nullptr || out == nullptr))) return -3;
  if (n == 0) return 0;
  const bool lds = K <= kCalibLdsKnots;
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  const int64_t work = vec ? (n + 3) / 4 : n;
  const unsigned grid = (unsigned)std::min<int64_t>((work + kCalibBlock - 1) / kCalibBlock, kCalibMaxBlocks);
  const size_t bytes = lds ? (size_t)K * (sizeof(double) + sizeof(float)) : 0;
  const auto fn = lds ? (vec ? k_calib_apply<true, true> : k_calib_apply<true, false>)
                      : (vec ? k_calib_apply<false, true> : k_calib_apply<false, false>);
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kCalibBlock), bytes, stream, x, n, xk, vk, K, out);
  CK_LAUNCH();
  return 0;
}

// p: float32 [n] in [0, 1]; y: float32 [n] (positive: > 0.5); wq: int32 [n] in [0, 2^20] or null (1 per row);
// edges: float32 [B - 1] ascending interior edges; out: int64 [3, B], added to. All on the device.
COBALT_API int cobalt_reliability_sums(const float* p, const float* y, const int32_t* wq, int64_t n,
                                       const float* edges, int B, int64_t* out, hipStream_t stream) {
  if (n < 0) return -1;
  if (B < 1 || B > kRelMaxBins) return -2;
  if (out == nullptr || (n > 0 && (p == nullptr || y == nullptr))) return -3;
  if (B > 1 && edges == nullptr) return -4;
  if (n == 0) return 0;
  const bool ldsc = B <= kRelLdsBins;
  const int64_t ntiles = (n + kRelTileRows - 1) / kRelTileRows;
  const int64_t tpb = (ntiles + kRelMaxBlocks - 1) / kRelMaxBlocks;
  const int64_t gx = (ntiles + tpb - 1) / tpb;
  const size_t bytes = ldsc ? (size_t)B * 16 + (size_t)(B - 1) * 4 : 0;
  const auto fn = wq ? (ldsc ? k_rel_sums<true, true> : k_rel_sums<true, false>)
                     : (ldsc ? k_rel_sums<false, true> : k_rel_sums<false, false>);
  hipLaunchKernelGGL(fn, dim3((unsigned)gx), dim3(kRelBlock), bytes, stream, p, y, wq, n, edges, B,
                     reinterpret_cast<unsigned long long*>(out), (int)tpb);
  CK_LAUNCH();
  return 0;
}
