// Integrated gradients of the MLP challenger against a background set (K31b): the network's
// counterpart of interventional TreeSHAP (`explain/nn.py MLPExplainer`).
//
//   phi[n][i] = 1/B sum_b (x_n[i] - z_b[i]) 1/M sum_m dF/dx_i (z_b + alpha_m (x_n - z_b)),
//   alpha_m = (m + 1/2) / M,  F = the logit, or sigmoid(logit) in probability mode.
//
// k_mlp_ig: one wave owns one explained row and walks its B * M quadrature points in the fixed
// order c = b * M + m, 32 consecutive points (one tile = the MFMA N dimension) at a time, so pairs
// share a tile when M < 32 and a pair spans tiles when M > 32. A row's result depends on (B, M)
// alone: not on N, its position in the batch, the grid, or any other row.
//   * The points are built in registers from x, z_b and alpha_m (fp32 fma); the next tile's z rows
//     are fetched while this tile computes. Nothing of size N x B x M exists in memory.
//   * Forward: k_mlp_forward_mfma's transposed chain on v_mfma_f32_32x32x2_f32 (hT = W^T . xT,
//     accumulators feed the next layer's B operand as they are). Only the three ReLU gate masks
//     (64 + 16 + 8 bits per lane) and the logit survive it.
//   * Backward to the input, the same trick with the weights in the other orientation:
//     d3 = W4 * gate3 (VALU), d2T = W3 . d3T (8 MFMAs), d1T = W2 . d2T (64), gT = W1 . d1T (rows =
//     features padded to 32, K = 128: 64), each gated by its mask; the K steps again walk the
//     hidden units in accumulator-register order. 4 S1 + 80 + 136 MFMAs per 32 points (256 at
//     F = 20). In probability mode the gradient column is scaled by p (1 - p) of its point.
//   * Both orientations of the weights are permuted once per workgroup into LDS as
//     [step / 4][lane][step % 4] (one conflict-free ds_read_b128 per 4 MFMAs): 65 KB at F = 20.
//   * Reduction: the tile's gradient [feature][point] and its z values go through a per-wave LDS
//     tile; lane f then walks the 32 points in order in fp64: a pair's M columns are summed,
//     multiplied by (x[f] - z_b[f]) (exact in fp64) and added to the row's accumulator, b ascending.
//     No atomics, no cross-wave sums: the same bits on every run.
// 8 waves per workgroup share the weight image (2 waves per SIMD); a row is one wave's work, so a
// batch of few rows against a large background uses few CUs.
#include "common.h"
#include <algorithm>

namespace {
constexpr int H1 = 128, H2 = 32, H3 = 16;
constexpr int kMaxF = 32, kS1Max = kMaxF / 2;
constexpr int kMaxSteps = 4096;          // alpha_m = (m + 1/2) / M stays far from fp32's resolution
constexpr int kMaxBackground = 1 << 24;  // B * M fits 2^36: int64 column counter
constexpr int kIgThreads = 512, kIgWaves = kIgThreads / 64;
constexpr int kPad = 33;                 // row pitch of the per-wave [feature][point] tiles
constexpr int kScratch = 2 * 32 * kPad;  // gradient tile + z tile

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

struct IgLayout {
  int A1, A2, A3, R3, R2, R1, b1, b2, b3, w4, b4, scratch, total;
};
__host__ __device__ constexpr IgLayout ig_layout(int S1) {
  IgLayout L{};
  int o = 0;
  L.A1 = o;  o += S1 * 256;   // forward: W1^T, features split over the lane halves
  L.A2 = o;  o += 16 * 256;   // forward: W2^T
  L.A3 = o;  o += 4 * 256;    // forward: W3^T, rows padded to 32
  L.R3 = o;  o += 2 * 256;    // backward: W3, K = 16 units of layer 3
  L.R2 = o;  o += 16 * 256;   // backward: W2, 4 row tiles x K = 32
  L.R1 = o;  o += 16 * 256;   // backward: W1, rows padded to 32, K = 128
  L.b1 = o;  o += H1;
  L.b2 = o;  o += H2;
  L.b3 = o;  o += 32;         // padded (zeros)
  L.w4 = o;  o += 32;         // padded (zeros)
  L.b4 = o;  o += 4;
  L.scratch = o;  o += kIgWaves * kScratch;
  L.total = o;
  return L;
}
static_assert(ig_layout(kS1Max).total * sizeof(float) <= 160 * 1024, "IG LDS image exceeds 160 KB");

// accumulator register v of lane half hi holds output row rowD(v, hi); K step s of the next MFMA
// reads register s, i.e. hidden unit 32 (s >> 4) + rowD(s & 15, hi)
__device__ __forceinline__ int rowD(int v, int hi) { return (v & 3) + 8 * (v >> 2) + 4 * hi; }
__device__ __forceinline__ int hid_of(int s, int hi) { return 32 * (s >> 4) + rowD(s & 15, hi); }

__device__ __forceinline__ void load_bias(f32x16& acc, const float* b, int hi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(b + 8 * q + 4 * hi);
    acc[4 * q + 0] = v.x;
    acc[4 * q + 1] = v.y;
    acc[4 * q + 2] = v.z;
    acc[4 * q + 3] = v.w;
  }
}

__device__ __forceinline__ uint32_t gate_mask(const f32x16& acc) {
  uint32_t m = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) m |= acc[v] > 0.0f ? (1u << v) : 0u;
  return m;
}

__global__ __launch_bounds__(kIgThreads) void k_mlp_ig(const float* __restrict__ X, int64_t ldx, int64_t N,
                                                       const float* __restrict__ Z, int64_t ldz, int B, int M, int F,
                                                       const float* __restrict__ params, int prob,
                                                       double* __restrict__ phi) {
  extern __shared__ float4 smv[];
  float* sm = reinterpret_cast<float*>(smv);
  const int S1 = (F + 1) >> 1;
  const IgLayout L = ig_layout(S1);
  {
    const float* W1 = params;
    const float* gb1 = W1 + F * H1;
    const float* W2 = gb1 + H1;
    const float* gb2 = W2 + H1 * H2;
    const float* W3 = gb2 + H2;
    const float* gb3 = W3 + H2 * H3;
    const float* W4 = gb3 + H3;
    const float* gb4 = W4 + H3;
    const int t0 = threadIdx.x;
    for (int e = t0; e < S1 * 256; e += kIgThreads) {
      const int s = e >> 8, l = (e >> 2) & 63, t = e & 3;
      const int k = (l >> 5) * S1 + s;
      sm[L.A1 + e] = k < F ? W1[k * H1 + 32 * t + (l & 31)] : 0.0f;
    }
    for (int e = t0; e < 16 * 256; e += kIgThreads) {
      const int l = (e >> 2) & 63, li = l & 31, hi = l >> 5;
      const int s = ((e >> 8) << 2) | (e & 3);       // forward: K step 0..63 of layer 2
      const int t = e >> 10, sb = (((e >> 8) & 3) << 2) | (e & 3);  // backward: row tile, K step 0..15
      sm[L.A2 + e] = W2[hid_of(s, hi) * H2 + li];
      sm[L.R2 + e] = W2[(32 * t + li) * H2 + rowD(sb, hi)];
      sm[L.R1 + e] = li < F ? W1[li * H1 + 32 * t + rowD(sb, hi)] : 0.0f;
    }
    for (int e = t0; e < 4 * 256; e += kIgThreads) {
      const int l = (e >> 2) & 63, s = ((e >> 8) << 2) | (e & 3);
      sm[L.A3 + e] = (l & 31) < H3 ? W3[hid_of(s, l >> 5) * H3 + (l & 31)] : 0.0f;
    }
    for (int e = t0; e < 2 * 256; e += kIgThreads) {
      const int l = (e >> 2) & 63, s = ((e >> 8) << 2) | (e & 3);  // K step 0..7: unit rowD(s, hi) < 16
      sm[L.R3 + e] = W3[(l & 31) * H3 + rowD(s, l >> 5)];
    }
    for (int e = t0; e < H1; e += kIgThreads) sm[L.b1 + e] = gb1[e];
    if (t0 < 32) {
      sm[L.b2 + t0] = gb2[t0];
      sm[L.b3 + t0] = t0 < H3 ? gb3[t0] : 0.0f;
      sm[L.w4 + t0] = t0 < H3 ? W4[t0] : 0.0f;
    }
    if (t0 == 0) sm[L.b4] = gb4[0];
    for (int e = t0; e < kIgWaves * kScratch; e += kIgThreads) sm[L.scratch + e] = 0.0f;
  }
  __syncthreads();
  const float4* A1v = reinterpret_cast<const float4*>(sm + L.A1);
  const float4* A2v = reinterpret_cast<const float4*>(sm + L.A2);
  const float4* A3v = reinterpret_cast<const float4*>(sm + L.A3);
  const float4* R3v = reinterpret_cast<const float4*>(sm + L.R3);
  const float4* R2v = reinterpret_cast<const float4*>(sm + L.R2);
  const float4* R1v = reinterpret_cast<const float4*>(sm + L.R1);
  const float* b1 = sm + L.b1;
  const float* b2 = sm + L.b2;
  const float* b3 = sm + L.b3;
  const float* w4 = sm + L.w4;
  const float bias4 = sm[L.b4];

  const int lane = threadIdx.x & 63, hi = lane >> 5, col = lane & 31;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* Gs = sm + L.scratch + wv * kScratch;  // [feature][point] gradient of the tile
  float* Zs = Gs + 32 * kPad;                  // [feature][point] background value of the point's pair
  const int kbase = hi * S1;
  const int nk = max(0, min(S1, F - kbase));   // features this lane half feeds to layer 1
  const bool fok = col < F;                    // the reduction's lane -> feature col
  const int64_t total = (int64_t)B * M;        // quadrature points of one row
  const int adv_b = 32 / M, adv_m = 32 % M;    // (pair, step) of a lane's point 32 columns on
  const double denom = (double)B * (double)M;

  for (int64_t n = (int64_t)blockIdx.x * kIgWaves + wv; n < N; n += (int64_t)gridDim.x * kIgWaves) {
    float xr[kS1Max];
#pragma unroll
    for (int s = 0; s < kS1Max; ++s) xr[s] = s < nk ? X[n * ldx + kbase + s] : 0.0f;
    const float xf = fok ? X[n * ldx + col] : 0.0f;
    int bl = col / M, ml = col - bl * M;  // this lane's point of the coming tile
    bool okn = col < total;
    float zn[kS1Max];
#pragma unroll
    for (int s = 0; s < kS1Max; ++s) zn[s] = (okn && s < nk) ? Z[(int64_t)bl * ldz + kbase + s] : 0.0f;
    double acc = 0.0, pair_sum = 0.0, diff = 0.0;
    int mw = 0;  // step of the reduction's walk inside its pair (wave-uniform)

    for (int64_t base = 0; base < total; base += 32) {
      // ---- the tile's 32 points; columns past the row's last point carry zeros and are not read
      const bool ok = okn;
      const float alpha = ((float)ml + 0.5f) / (float)M;
      float xv[kS1Max];
#pragma unroll
      for (int s = 0; s < kS1Max; ++s) {
        const float z = zn[s];
        xv[s] = ok ? fmaf(alpha, xr[s] - z, z) : 0.0f;
        if (s < nk) Zs[(kbase + s) * kPad + col] = z;
      }
      ml += adv_m;
      bl += adv_b;
      if (ml >= M) {
        ml -= M;
        ++bl;
      }
      okn = base + 32 + col < total;
#pragma unroll
      for (int s = 0; s < kS1Max; ++s) zn[s] = (okn && s < nk) ? Z[(int64_t)bl * ldz + kbase + s] : 0.0f;

      // ---- forward (k_mlp_forward_mfma's chain), keeping the gate masks
      uint32_t m1[4], m2, m3;
      f32x16 acc2;
      {
        f32x16 a1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) load_bias(a1[t], b1 + 32 * t, hi);
#pragma unroll
        for (int s = 0; s < kS1Max; ++s) {
          if (s < S1) {
            const float4 a = A1v[s * 64 + lane];
            a1[0] = MFMA32(a.x, xv[s], a1[0]);
            a1[1] = MFMA32(a.y, xv[s], a1[1]);
            a1[2] = MFMA32(a.z, xv[s], a1[2]);
            a1[3] = MFMA32(a.w, xv[s], a1[3]);
          }
        }
        load_bias(acc2, b2, hi);
#pragma unroll
        for (int sg = 0; sg < 16; ++sg) {
          const float4 a = A2v[sg * 64 + lane];
          const int t = sg >> 2, v = (sg & 3) * 4;
          acc2 = MFMA32(a.x, fmaxf(a1[t][v + 0], 0.0f), acc2);
          acc2 = MFMA32(a.y, fmaxf(a1[t][v + 1], 0.0f), acc2);
          acc2 = MFMA32(a.z, fmaxf(a1[t][v + 2], 0.0f), acc2);
          acc2 = MFMA32(a.w, fmaxf(a1[t][v + 3], 0.0f), acc2);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) m1[t] = gate_mask(a1[t]);
      }
      m2 = gate_mask(acc2);
      f32x16 acc3;
      load_bias(acc3, b3, hi);
#pragma unroll
      for (int sg = 0; sg < 4; ++sg) {
        const float4 a = A3v[sg * 64 + lane];
        acc3 = MFMA32(a.x, fmaxf(acc2[4 * sg + 0], 0.0f), acc3);
        acc3 = MFMA32(a.y, fmaxf(acc2[4 * sg + 1], 0.0f), acc3);
        acc3 = MFMA32(a.z, fmaxf(acc2[4 * sg + 2], 0.0f), acc3);
        acc3 = MFMA32(a.w, fmaxf(acc2[4 * sg + 3], 0.0f), acc3);
      }
      m3 = gate_mask(acc3) & 0xffu;  // units 0..15 are registers 0..7 of the two halves
      float gscale = 1.0f;
      if (prob) {
        float z = 0.0f;
#pragma unroll
        for (int v = 0; v < 8; ++v) z = fmaf(w4[rowD(v, hi)], fmaxf(acc3[v], 0.0f), z);
        z += __shfl_xor(z, 32);
        z += bias4;
        const float e = expf(-fabsf(z));  // p (1 - p) = e / (1 + e)^2, no cancellation at either tail
        gscale = e / ((1.0f + e) * (1.0f + e));
      }

      // ---- backward to the input
      float d3[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) d3[v] = (m3 >> v) & 1u ? w4[rowD(v, hi)] : 0.0f;
      f32x16 a2d = {};
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        const float4 a = R3v[sg * 64 + lane];
        a2d = MFMA32(a.x, d3[4 * sg + 0], a2d);
        a2d = MFMA32(a.y, d3[4 * sg + 1], a2d);
        a2d = MFMA32(a.z, d3[4 * sg + 2], a2d);
        a2d = MFMA32(a.w, d3[4 * sg + 3], a2d);
      }
      float d2[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) d2[v] = (m2 >> v) & 1u ? a2d[v] : 0.0f;
      f32x16 g = {};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f32x16 a1d = {};
#pragma unroll
        for (int sg = 0; sg < 4; ++sg) {
          const float4 a = R2v[(4 * t + sg) * 64 + lane];
          a1d = MFMA32(a.x, d2[4 * sg + 0], a1d);
          a1d = MFMA32(a.y, d2[4 * sg + 1], a1d);
          a1d = MFMA32(a.z, d2[4 * sg + 2], a1d);
          a1d = MFMA32(a.w, d2[4 * sg + 3], a1d);
        }
#pragma unroll
        for (int sg = 0; sg < 4; ++sg) {
          const float4 a = R1v[(4 * t + sg) * 64 + lane];
          const uint32_t mt = m1[t] >> (4 * sg);
          g = MFMA32(a.x, mt & 1u ? a1d[4 * sg + 0] : 0.0f, g);
          g = MFMA32(a.y, mt & 2u ? a1d[4 * sg + 1] : 0.0f, g);
          g = MFMA32(a.z, mt & 4u ? a1d[4 * sg + 2] : 0.0f, g);
          g = MFMA32(a.w, mt & 8u ? a1d[4 * sg + 3] : 0.0f, g);
        }
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) Gs[rowD(v, hi) * kPad + col] = g[v] * gscale;

      // ---- reduction: lane f (both halves alike) walks the tile's points in order
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float gc[32], zc[32];
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        gc[c] = Gs[col * kPad + c];
        zc[c] = Zs[col * kPad + c];
      }
      const int ncol = (int)min((int64_t)32, total - base);
#pragma unroll
      for (int c = 0; c < 32; ++c) {
        if (c < ncol) {
          if (mw == 0) diff = (double)xf - (double)zc[c];
          pair_sum += (double)gc[c];
          if (++mw == M) {
            acc += diff * pair_sum;
            pair_sum = 0.0;
            mw = 0;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (hi == 0 && fok) phi[n * F + col] = acc / denom;
  }
}
#undef MFMA32
}  // namespace

COBALT_API int cobalt_mlp_ig_max_features() { return kMaxF; }
COBALT_API int cobalt_mlp_ig_max_steps() { return kMaxSteps; }
COBALT_API int cobalt_mlp_ig_max_background() { return kMaxBackground; }

// phi [n, F] float64 (contiguous) <- integrated gradients of the fp32 rows X [n, F] (row stride ldx)
// against the background rows Z [B, F] (row stride ldz) with n_steps midpoint steps per pair.
COBALT_API int cobalt_mlp_ig(const float* X, int64_t ldx, int64_t n, const float* Z, int64_t ldz, int64_t B,
                             int n_steps, int F, const float* params, int probability, double* phi,
                             hipStream_t stream) {
  if (F < 1 || F > kMaxF) return -1;
  if (B < 1 || B > kMaxBackground) return -2;
  if (n_steps < 1 || n_steps > kMaxSteps) return -3;
  if (n < 1) return 0;
  const size_t lds = (size_t)ig_layout((F + 1) / 2).total * sizeof(float);  // 131 KB at F = 20
  CK(hipFuncSetAttribute((const void*)k_mlp_ig, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int dev = 0, cus = 0;
  CK(hipGetDevice(&dev));
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int64_t groups = (n + kIgWaves - 1) / kIgWaves;
  const int grid = (int)std::min<int64_t>(groups, std::max(cus, 1));  // one workgroup per CU (LDS)
  hipLaunchKernelGGL(k_mlp_ig, dim3(grid), dim3(kIgThreads), lds, stream, X, ldx, n, Z, ldz, (int)B, n_steps, F,
                     params, probability, phi);
  CK_LAUNCH();
  return 0;
}
