// The counter-based generator of the resampling kernels (gfx950): Philox4x32-10 and the Poisson(1) count of one
// of its output words. The host form is metrics/bootstrap.py (philox4x32_10, poisson1_count); the two give the
// same bits.
#pragma once
#include "common.h"

namespace cobalt {

constexpr uint32_t kPhiloxMul0 = 0xD2511F53u, kPhiloxMul1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxWeyl0 = 0x9E3779B9u, kPhiloxWeyl1 = 0xBB67AE85u;
constexpr int kPoisson1MaxCount = 12;  // poisson1 returns 0 .. 12

// Philox4x32-10 on counter x[0 .. 3] and key (k0, k1), in place.
__device__ __forceinline__ void philox4x32_10(uint32_t x[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(kPhiloxMul0, x[0]), l0 = kPhiloxMul0 * x[0];
    const uint32_t h1 = __umulhi(kPhiloxMul1, x[2]), l1 = kPhiloxMul1 * x[2];
    x[0] = h1 ^ x[1] ^ k0;
    x[1] = l1;
    x[2] = h0 ^ x[3] ^ k1;
    x[3] = l0;
    k0 += kPhiloxWeyl0;
    k1 += kPhiloxWeyl1;
  }
}

// #{k : u >= floor(2^32 PoissonCDF(k; 1))}, k = 0 .. 11: a Poisson(1) count from a uniform 32-bit word.
__device__ __forceinline__ uint32_t poisson1(uint32_t u) {
  return (u >= 0x5e2d58d8u) + (u >= 0xbc5ab1b1u) + (u >= 0xeb715e1du) + (u >= 0xfb239797u) + (u >= 0xff1025f5u) +
         (u >= 0xffd90f3bu) + (u >= 0xfffa8b71u) + (u >= 0xffff540cu) + (u >= 0xffffed1fu) + (u >= 0xfffffe21u) +
         (u >= 0xffffffd4u) + (u >= 0xfffffffcu);
}

// The Poisson-bootstrap counts of ORIGINAL row i in the four replicates 4 q .. 4 q + 3: counter (i, q, 0, 0),
// key (seed lo, seed hi), one count per output word.
__device__ __forceinline__ void bootstrap_row_counts(uint32_t i, uint32_t q, uint32_t k0, uint32_t k1, uint32_t c[4]) {
  uint32_t x[4] = {i, q, 0u, 0u};
  philox4x32_10(x, k0, k1);
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = poisson1(x[j]);
}

}  // namespace cobalt
