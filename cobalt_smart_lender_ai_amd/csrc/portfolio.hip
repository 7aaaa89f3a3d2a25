// Monte-Carlo loss distribution of a loan book under the Gaussian-copula factor model (gfx950): per scenario and
// segment the summed loss and the number of defaults. The primitive under portfolio/loss.py, whose
// portfolio_sums_host is the definition and whose portfolio_sums_tiled_host is this file's decomposition on the
// host. Every step of a draw is integer arithmetic on inputs prepared once in fp64 on the host, so the host and
// the device give the same bits; the sums are 64-bit integers added in a fixed order, no atomics anywhere.
//
// Input. One 16-byte record per loan: the ORIGINAL loan index (x), the probit point Q (y, int32, |Q| <= 2^30),
// the loss amount L (z, uint32) and the sector (w). A: int32 [S, K], the scenario offsets of this call's
// scenarios (|A| <= 2^29). T: int64 [8193], floor(2^32 Phi(-8 + j 2^-9)) with T[0] = 0 and T[8192] = 2^32; the
// device never evaluates erfc.
//
// A draw. X = clamp(Q - A[s, sector] + 8 2^20, 0, 16 2^20), j = X >> 11, f = X & 2047,
// thr = T[j] + (((T[min(j + 1, 8192)] - T[j]) f) >> 11); u = word (s & 3) of Philox4x32-10(counter (index, s >>
// 2, 0, kPfDomain), key (seed lo, seed hi)); default iff u < thr in 64 bits. One Philox call serves the four
// scenarios a thread owns. The draw never depends on where the record stands, so sorting and padding the book
// cannot change a sum.
//
// Design choices
//  * k_pf_tiles: blockIdx.x is a tile of kPfTileRows consecutive records, blockIdx.y a group of kPfBlockScen
//    scenarios. The tile's records are staged in LDS once; every lane then walks them IN ORDER and reads the same
//    record: the LDS read is a broadcast and the record goes to scalar registers. What differs between lanes is
//    the Philox counter and the offsets.
//  * T lives in LDS as 32-bit words for the gather (two reads per draw). T[8192] = 2^32 is stored as 0, twice
//    (entries 8192 and 8193), so that j + 1 needs no clamp: the 32-bit difference T[j + 1] - T[j] is right
//    modulo 2^32 (it is below 2^22 everywhere), and j = 8192, the only index whose threshold is 2^32, is set
//    apart by a compare. With one sector the lane's four offsets sit in registers; with more, the block's
//    offsets are staged in LDS as [sector][scenario] and a lane reads its four with one 16-byte read.
//  * Per tile the loss is 64-bit, the defaults 32-bit (at most kPfTileRows). Records are [tile][field][scenario]:
//    a lane stores four consecutive int64.
//  * Segments: the caller sorts the records by segment and pads every segment to whole tiles with records that
//    never default (Q = -2^30, L = 0), so a tile belongs to one segment. k_pf_stitch, one thread per (segment,
//    scenario), adds the tiles tile_seg[g] .. tile_seg[g + 1] in order.
//  * Out-of-range Q, A and sector values are clamped where they are staged: no input can index outside T or A.
//  * Refusals come before any launch: -1 n < 1, -2 n > 2^28, -3 scenarios < 1 or > 2^20, -4 rep0 negative or no
//    multiple of 4, -5 a null pointer, -6 workspace too small, -7 ld < scenarios, -8 K outside 1 .. 16, -9 G
//    outside 1 .. 64, -10 the largest sector id the caller states is negative or >= K, -11 tile_seg is not a
//    non-decreasing table from 0 to the number of tiles.
#include "common.h"

using namespace cobalt;

namespace {
constexpr int kPfTileRows = 1024;
constexpr int kPfBlock = 256;
constexpr int kPfScenPerThread = 4;  // one Philox call
constexpr int kPfBlockScen = kPfBlock * kPfScenPerThread;
constexpr int kPfStitchBlock = 256;
constexpr int64_t kPfMaxRows = (int64_t)1 << 28;
constexpr int kPfMaxScen = 1 << 20;
constexpr int kPfMaxSectors = 16;
constexpr int kPfMaxSegments = 64;
constexpr int kPfTableSteps = 8192;
constexpr int kPfTableLds = kPfTableSteps + 4;  // T[0 .. 8192], one more copy of the last, padding to 16 bytes
constexpr int kPfShift = 11;
constexpr int kPfOffset = 8 << 20, kPfXMax = 16 << 20;
constexpr int kPfQClamp = 1 << 30, kPfAClamp = 1 << 29;
constexpr uint32_t kPfDomain = 0x504C4F53u;
static_assert(kPfBlockScen % 4 == 0 && (kPfTableLds * 4) % 16 == 0, "16-byte aligned LDS sections");

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct PfSegTable {
  int32_t first[kPfMaxSegments + 1];  // segment g owns tiles first[g] .. first[g + 1]
};

constexpr size_t pf_lds_bytes(int K) {
  return (size_t)kPfTileRows * 16 + (size_t)kPfTableLds * 4 + (K > 1 ? (size_t)K * kPfBlockScen * 4 : 0);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
}  // namespace

// Block (t, g): tile t of the records, scenarios [g * kPfBlockScen, ...) of this call; a thread owns four.
// recs: int64 [tiles][2][Sp], Sp = scenarios rounded up to 4 (a thread stores all four of its scenarios; those
// past S land in the padding).
template <bool SINGLE>
__global__ __launch_bounds__(kPfBlock) void k_pf_tiles(const uint4* __restrict__ loans, int64_t n,
                                                       const int32_t* __restrict__ A, int K,
                                                       const int64_t* __restrict__ table, uint32_t q0, int S,
                                                       uint32_t k0, uint32_t k1, int64_t* __restrict__ recs,
                                                       int64_t Sp) {
  extern __shared__ uint4 s_pf[];
  uint4* s_rec = s_pf;                                                  // [kPfTileRows]
  uint32_t* s_T = reinterpret_cast<uint32_t*>(s_rec + kPfTileRows);     // [kPfTableLds]
  int32_t* s_A = reinterpret_cast<int32_t*>(s_T + kPfTableLds);         // [K][kPfBlockScen], K > 1 only
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t row0 = tile * kPfTileRows;
  const int rows = (int)min((int64_t)kPfTileRows, n - row0);
  const int s0 = (int)blockIdx.y * kPfBlockScen;
  for (int r = tid; r < rows; r += kPfBlock) {
    uint4 v = loans[row0 + r];
    v.y = (uint32_t)clampi((int)v.y, -kPfQClamp, kPfQClamp);
    v.w = min(v.w, (uint32_t)(K - 1));
    s_rec[r] = v;
  }
  for (int j = tid; j < kPfTableSteps + 2; j += kPfBlock) s_T[j] = (uint32_t)table[min(j, kPfTableSteps)];
  if constexpr (!SINGLE) {
    for (int e = tid; e < K * kPfBlockScen; e += kPfBlock) {
      const int k = e / kPfBlockScen, s = s0 + (e - k * kPfBlockScen);
      s_A[e] = s < S ? clampi(A[(int64_t)s * K + k], -kPfAClamp, kPfAClamp) : 0;
    }
  }
  __syncthreads();
  const int r0 = s0 + tid * kPfScenPerThread;
  if (r0 >= S) return;
  const uint32_t q = q0 + (uint32_t)(r0 >> 2);
  int a[4] = {0, 0, 0, 0};
  if constexpr (SINGLE) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (r0 + j < S) a[j] = clampi(A[r0 + j], -kPfAClamp, kPfAClamp);
  }

  uint64_t loss[4] = {0, 0, 0, 0};
  uint32_t cnt[4] = {0, 0, 0, 0};
  for (int r = 0; r < rows; ++r) {
    const uint4 rec = s_rec[r];  // every lane reads the same record
    const uint32_t idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x);
    const int Q = __builtin_amdgcn_readfirstlane((int)rec.y);
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.z);
    if constexpr (!SINGLE) {
      const int sec = __builtin_amdgcn_readfirstlane((int)rec.w);
      const int4 v = *reinterpret_cast<const int4*>(s_A + sec * kPfBlockScen + tid * kPfScenPerThread);
      a[0] = v.x;
      a[1] = v.y;
      a[2] = v.z;
      a[3] = v.w;
    }
    uint32_t x0 = idx, x1 = q, x2 = 0u, x3 = kPfDomain, c0 = k0, c1 = k1;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const uint32_t h0 = __umulhi(kPhiloxM0, x0), l0 = kPhiloxM0 * x0;
      const uint32_t h1 = __umulhi(kPhiloxM1, x2), l1 = kPhiloxM1 * x2;
      x0 = h1 ^ x1 ^ c0;
      x1 = l1;
      x2 = h0 ^ x3 ^ c1;
      x3 = l0;
      c0 += kPhiloxW0;
      c1 += kPhiloxW1;
    }
    const uint32_t u[4] = {x0, x1, x2, x3};
    const int base = Q + kPfOffset;  // |Q| <= 2^30 and |a| <= 2^29: no 32-bit overflow below
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int X = clampi(base - a[j], 0, kPfXMax);
      const uint32_t tj = (uint32_t)X >> kPfShift, f = (uint32_t)X & ((1u << kPfShift) - 1u);
      const uint32_t t0 = s_T[tj], d = s_T[tj + 1] - t0;
      const uint64_t thr =
          tj >= (uint32_t)kPfTableSteps ? (uint64_t)1 << 32 : (uint64_t)t0 + (((uint64_t)d * f) >> kPfShift);
      const bool dflt = (uint64_t)u[j] < thr;
      loss[j] += dflt ? (uint64_t)L : 0ull;
      cnt[j] += dflt ? 1u : 0u;
    }
  }
  int64_t* rec = recs + tile * 2 * Sp + r0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rec[j] = (int64_t)loss[j];
    rec[Sp + j] = (int64_t)cnt[j];
  }
}

// One thread per (segment, scenario): the records of the segment's tiles, in order, into out [2][G][ld].
__global__ __launch_bounds__(kPfStitchBlock) void k_pf_stitch(const int64_t* __restrict__ recs, PfSegTable seg,
                                                              int G, int S, int64_t Sp, int64_t* __restrict__ out,
                                                              int64_t ld) {
  const int s = blockIdx.x * kPfStitchBlock + threadIdx.x;
  const int g = blockIdx.y;
  if (s >= S) return;
  int64_t loss = 0, cnt = 0;
  for (int64_t t = seg.first[g]; t < seg.first[g + 1]; ++t) {
    loss += recs[t * 2 * Sp + s];
    cnt += recs[(t * 2 + 1) * Sp + s];
  }
  out[(int64_t)g * ld + s] = loss;
  out[((int64_t)G + g) * ld + s] = cnt;
}

COBALT_API int cobalt_portfolio_tile_rows() { return kPfTileRows; }
COBALT_API int cobalt_portfolio_block_scenarios() { return kPfBlockScen; }
COBALT_API int64_t cobalt_portfolio_max_rows() { return kPfMaxRows; }

// Bytes of workspace for n records and `scenarios` scenarios in one call, or the refusal of cobalt_portfolio for
// these shapes.
COBALT_API int64_t cobalt_portfolio_workspace_bytes(int64_t n, int scenarios) {
  if (n < 1) return -1;
  if (n > kPfMaxRows) return -2;
  if (scenarios < 1 || scenarios > kPfMaxScen) return -3;
  const int64_t tiles = (n + kPfTileRows - 1) / kPfTileRows;
  const int64_t Sp = ((int64_t)scenarios + 3) / 4 * 4;
  return tiles * 2 * Sp * 8;
}

// loans: uint4 [n] (layout above), sorted by segment and padded so that every tile belongs to one segment;
// tile_seg: HOST int32 [G + 1], segment g owns tiles tile_seg[g] .. tile_seg[g + 1] (tile_seg[G] is the number of
// tiles); sector_max: the largest sector id in the records, as the caller found it (the kernel clamps, so a
// wrong statement cannot read outside A). A: int32 [scenarios, K]; table: int64 [8193]. Scenarios rep0 .. rep0 +
// scenarios - 1 (rep0 a multiple of 4) go to columns 0 .. scenarios - 1 of out (int64 [2, G, ld]: loss,
// defaults). Everything runs on `stream`; workspace is scratch of at least cobalt_portfolio_workspace_bytes and
// may be reused by the next call on the same stream.
COBALT_API int cobalt_portfolio(const void* loans, int64_t n, const int32_t* A, int K, int sector_max,
                                const int64_t* table, const int32_t* tile_seg, int G, int64_t rep0, int scenarios,
                                uint64_t seed, void* workspace, int64_t workspace_bytes, int64_t* out, int64_t ld,
                                hipStream_t stream) {
  const int64_t need = cobalt_portfolio_workspace_bytes(n, scenarios);
  if (need < 0) return (int)need;
  if (rep0 < 0 || (rep0 & 3) != 0 || rep0 + scenarios > ((int64_t)1 << 32)) return -4;
  if (loans == nullptr || A == nullptr || table == nullptr || tile_seg == nullptr || workspace == nullptr ||
      out == nullptr)
    return -5;
  if (workspace_bytes < need) return -6;
  if (ld < scenarios) return -7;
  if (K < 1 || K > kPfMaxSectors) return -8;
  if (G < 1 || G > kPfMaxSegments) return -9;
  if (sector_max < 0 || sector_max >= K) return -10;
  const int64_t tiles = (n + kPfTileRows - 1) / kPfTileRows;
  PfSegTable seg;
  for (int g = 0; g <= kPfMaxSegments; ++g) seg.first[g] = tile_seg[g < G ? g : G];
  if (seg.first[0] != 0 || seg.first[G] != tiles) return -11;
  for (int g = 0; g < G; ++g)
    if (seg.first[g + 1] < seg.first[g]) return -11;
  const int64_t Sp = ((int64_t)scenarios + 3) / 4 * 4;
  int64_t* recs = static_cast<int64_t*>(workspace);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32), q0 = (uint32_t)(rep0 >> 2);
  const dim3 grid((unsigned)tiles, (unsigned)((scenarios + kPfBlockScen - 1) / kPfBlockScen));
  const dim3 sgrid((unsigned)((scenarios + kPfStitchBlock - 1) / kPfStitchBlock), (unsigned)G);
  const size_t lds = pf_lds_bytes(K);
  const auto tiles_fn = K == 1 ? k_pf_tiles<true> : k_pf_tiles<false>;
  if (lds > 64 * 1024)
    CK(hipFuncSetAttribute((const void*)tiles_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(tiles_fn, grid, dim3(kPfBlock), lds, stream, static_cast<const uint4*>(loans), n, A, K, table,
                     q0, scenarios, k0, k1, recs, Sp);
  CK_LAUNCH();
  hipLaunchKernelGGL(k_pf_stitch, sgrid, dim3(kPfStitchBlock), 0, stream, recs, seg, G, scenarios, Sp, out, ld);
  CK_LAUNCH();
  return 0;
}
