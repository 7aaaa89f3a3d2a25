// The trainer's arithmetic that other kernels must reproduce bit for bit: the gradient quantiser and the
// node weight / gain expressions. gbdt.hip trains with them; refresh.hip recomputes a model's statistics on
// new rows and is only correct if it draws the trainer's exact bits. models/gbdt_host.py is the oracle
// (gradients_host, _thresh_l1, _calc_gain, _calc_weight).
#pragma once
#include "common.h"

namespace cobalt {

// Gradient fixed point (models/gbdt_host.py gradients_host is the oracle): |g| <= w_max and
// h <= w_max / 4 are scaled to 17 bits and rounded UNBIASED, q = floor(x * scale + u) with u ~ U[0,1)
// drawn from a per-(tree, global row) hash -- E[q] = x * scale, so small hessians are not flushed
// to 0 and rounding errors of histogram sums average out instead of accumulating a bias. The draw is
// deterministic (same trees on every device and rank count). Bounds: a <= 16384-row histogram block
// sums to |sum g| < 2^31 and sum h <= 2^31, so the packed u64 (signed g high, h low) never carries.
// Wide gradients (GbdtConfig::grad_bits 25): 25-bit magnitudes, summed in int64 cells (a 16384-row block
// < 2^39; 10M rows < 2^49, exact in the host oracle's float64 sums too).
constexpr int64_t kGClip = (1 << 17) - 1, kHClip = 1 << 17;
constexpr int64_t kGClipW = (1 << 25) - 1, kHClipW = 1 << 25;
constexpr uint64_t kDitherSalt = 0xD1B54A32D192ED03ull;

__host__ __device__ __forceinline__ uint64_t tree_key_of(uint64_t seed, int tree) {
  return splitmix64(seed ^ (0xA5A5A5A5ull + (uint64_t)tree * 0x632BE59BD9B4E019ull));
}

// dkey = splitmix64(tree_key_of(seed, tree) ^ kDitherSalt); grow = the row's global index.
__device__ __forceinline__ void quantize_gh(double g, double h, double gscale, double hscale, uint64_t dkey,
                                            int64_t grow, int64_t& gq, int64_t& hq, bool wide = false) {
  const uint64_t r = splitmix64(dkey ^ (uint64_t)grow);
  const double ug = (double)(uint32_t)(r >> 32) * (1.0 / 4294967296.0);
  const double uh = (double)(uint32_t)r * (1.0 / 4294967296.0);
  gq = (int64_t)floor(g * gscale + ug);
  hq = (int64_t)floor(h * hscale + uh);
  const int64_t gc = wide ? kGClipW : kGClip, hc = wide ? kHClipW : kHClip;
  gq = gq > gc ? gc : (gq < -gc ? -gc : gq);
  hq = hq > hc ? hc : (hq < 0 ? 0 : hq);
}

__device__ __forceinline__ double thresh_l1(double g, double alpha) {
  if (g > alpha) return g - alpha;
  if (g < -alpha) return g + alpha;
  return 0.0;
}

__device__ __forceinline__ double calc_gain(double g, double h, double lambda_, double alpha, double mcw) {
  if (h < mcw) return 0.0;
  const double t = alpha == 0.0 ? g : thresh_l1(g, alpha);
  return (t * t) / (h + lambda_);
}

__device__ __forceinline__ double calc_weight(double g, double h, double lambda_, double alpha, double mcw) {
  if (h < mcw || h <= 0.0) return 0.0;
  const double t = alpha == 0.0 ? g : thresh_l1(g, alpha);
  return -t / (h + lambda_);
}

}  // namespace cobalt
