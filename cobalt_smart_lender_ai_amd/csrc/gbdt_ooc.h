// ------------------------------------------------------------------------------------------
// External-memory training (BASELINE.json config "100M-row out-of-core GBDT with
// host-DRAM spill"). The quantised row records live in host memory as pages; per tree every page
// streams through k_ooc_page, which
//   * applies the previous tree to the rows' margins (margins / labels / weights stay on the device),
//   * computes binary:logistic g, h (fp64, as k_grad) and ghat = sqrt(g^2 + h^2),
//   * keeps a minimal-variance sample (MVS -- the sampler of XGBoost's gradient_based external
//     memory mode): row i with probability p_i = min(1, ghat_i / mu), its pair reweighted by 1/p_i
//     (unbiased histograms; |g/p|, h/p <= mu, so the fixed-point scales hold when mu <= w_max),
//   * compacts kept rows into the trainer's row records + feature-major bins (one wave-aggregated
//     claim per wave; the order is irrelevant because every histogram sum is an exact integer),
//   * counts ghat in kOocBins log-spaced bins (binary exponent x 16 mantissa steps, exact integer
//     counts -> the host derives the next mu deterministically, models/external.py).
// The in-core trainer then grows the tree on the sample (cobalt_gbdt_grow_sampled).
// ------------------------------------------------------------------------------------------
// Part of the trainer's one translation unit: csrc/gbdt.hip includes this file after the code it builds on
// (it is not self-contained).
#pragma once

constexpr int kOocBins = 2048;

__device__ __forceinline__ int ooc_bin(double v) {
  if (!(v > 0.0)) return 0;
  int e;
  const double f = frexp(v, &e);  // v = f * 2^e, f in [0.5, 1)
  const int b = (e + 64) * 16 + (int)floor((f - 0.5) * 32.0);
  return b < 1 ? 1 : (b >= kOocBins ? kOocBins - 1 : b);
}

// `ps` = page row stride in bytes: 32 (full row records) or the compact spill format, the F bins
// rounded up to 4 bytes (20 B for the 20 deployed features: 37% less PCIe traffic per tree -- the
// per-tree page stream is bound by the H2D copy).
__global__ __launch_bounds__(256) void k_ooc_page(const uint8_t* __restrict__ page, int ps, int64_t n, int64_t r0, int F,
                                                  const Node* __restrict__ prev, int max_nodes,
                                                  float* __restrict__ margin, const float* __restrict__ label,
                                                  const float* __restrict__ weight, uint64_t key, int64_t row_offset,
                                                  double mu, double gscale, double hscale, uint8_t* __restrict__ srec,
                                                  uint8_t* __restrict__ sbinsT, int64_t cap,
                                                  unsigned long long* __restrict__ counter,
                                                  unsigned int* __restrict__ hist) {
  __shared__ uint32_t s_meta[2047];
  __shared__ float s_leaf[2047];
  __shared__ unsigned int s_h[kOocBins];
  for (int i = threadIdx.x; i < kOocBins; i += blockDim.x) s_h[i] = 0u;
  if (prev != nullptr)
    for (int i = threadIdx.x; i < max_nodes; i += blockDim.x) {
      const Node nd = prev[i];
      s_meta[i] = node_meta(nd);
      s_leaf[i] = nd.leaf_value;
    }
  __syncthreads();
  const int lane = lane_id();
  // wave-uniform loop (ballots below): every lane of a wave iterates the same bases
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < n;
    bool keep = false;
    uint4 ra = make_uint4(0, 0, 0, 0), rb = make_uint4(0, 0, 0, 0);
    if (in) {
      if (ps == 32) {
        const uint4* rec = reinterpret_cast<const uint4*>(page + i * 32);
        ra = rec[0];
        rb = rec[1];
        rb.z = rb.w = 0u;  // (g, h) slot: rewritten below for kept rows
      } else {  // compact page: ps / 4 bin words, the rest of the record is zero padding
        const uint32_t* rw = reinterpret_cast<const uint32_t*>(page + i * ps);
        const int nw = ps >> 2;
        ra.x = rw[0];
        if (nw > 1) ra.y = rw[1];
        if (nw > 2) ra.z = rw[2];
        if (nw > 3) ra.w = rw[3];
        if (nw > 4) rb.x = rw[4];
        if (nw > 5) rb.y = rw[5];
      }
      float mf = margin[r0 + i];
      if (prev != nullptr) {
        int nx = 0;
        uint32_t m = s_meta[0];
        while (m & kMetaSplit) {
          const int f = m & 0xFFFF, q = f >> 2;
          const uint32_t word = q == 0 ? ra.x : q == 1 ? ra.y : q == 2 ? ra.z : q == 3 ? ra.w : q == 4 ? rb.x : rb.y;
          const uint32_t b = (word >> (8 * (f & 3))) & 0xffu;
          const bool left = meta_left(m, b);
          nx = 2 * nx + (left ? 1 : 2);
          m = s_meta[nx];
        }
        mf += s_leaf[nx];
        margin[r0 + i] = mf;
      }
      const double p = 1.0 / (1.0 + exp(-(double)mf));
      const double y = (double)label[r0 + i], w = (double)weight[r0 + i];
      const double g = (p - y) * w;
      const double h = fmax(p * (1.0 - p), 1e-16) * w;
      const double gh = sqrt(g * g + h * h);
      atomicAdd(&s_h[ooc_bin(gh)], 1u);
      if (mu > 0.0) {
        const double pk = gh >= mu ? 1.0 : gh / mu;
        keep = uniform01(splitmix64(key ^ (uint64_t)(row_offset + r0 + i))) < pk;
        if (keep) {
          int64_t gq = (int64_t)rint(g / pk * gscale), hq = (int64_t)rint(h / pk * hscale);
          gq = gq > 65536 ? 65536 : (gq < -65536 ? -65536 : gq);
          hq = hq > 65536 ? 65536 : (hq < 0 ? 0 : hq);
          rb.z = (uint32_t)hq;
          rb.w = (uint32_t)(int32_t)gq;
        }
      }
    }
    const uint64_t km = __ballot(keep);
    if (km) {
      const int leader = __ffsll((unsigned long long)km) - 1;
      unsigned long long b0 = 0;
      if (lane == leader) b0 = atomicAdd(counter, (unsigned long long)__popcll(km));
      b0 = (unsigned long long)readlane64((int64_t)b0, leader);
      if (keep) {
        const int64_t slot = (int64_t)b0 + mask_rank(km);
        if (slot < cap) {
          uint4* dst = reinterpret_cast<uint4*>(srec + slot * 32);
          dst[0] = ra;
          dst[1] = rb;
          for (int f = 0; f < F; ++f) {
            const int q = f >> 2;
            const uint32_t word = q == 0 ? ra.x : q == 1 ? ra.y : q == 2 ? ra.z : q == 3 ? ra.w : q == 4 ? rb.x : rb.y;
            sbinsT[(int64_t)f * cap + slot] = (uint8_t)((word >> (8 * (f & 3))) & 0xffu);
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kOocBins; i += blockDim.x)
    if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

COBALT_API int cobalt_ooc_page(const uint8_t* page, int page_stride, int64_t n, int64_t r0, int F, const void* prev,
                               int max_nodes,
                               float* margin, const float* label, const float* weight, uint64_t key,
                               int64_t row_offset, double mu, double gscale, double hscale, uint8_t* srec,
                               uint8_t* sbinsT, int64_t cap, unsigned long long* counter, unsigned int* hist,
                               hipStream_t stream) {
  if (F < 1 || F > 24 || max_nodes > 2047 || n < 0) return -3;  // 32-byte records only
  if (page_stride != 32 && (page_stride % 4 != 0 || page_stride < F || page_stride > 24)) return -3;
  if (n == 0) return 0;
  const int grid = std::max(1, std::min(ceil_div(n, 256), 256 * 8));
  hipLaunchKernelGGL(k_ooc_page, dim3(grid), dim3(256), 0, stream, page, page_stride, n, r0, F,
                     static_cast<const Node*>(prev),
                     max_nodes, margin, label, weight, key, row_offset, mu, gscale, hscale, srec, sbinsT, cap, counter,
                     hist);
  CK_LAUNCH();
  return 0;
}

COBALT_API int cobalt_ooc_bins() { return kOocBins; }
