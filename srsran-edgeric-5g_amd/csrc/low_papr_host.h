// Plan-time constants of the low-PAPR sequences of low_papr_device.h, shared by the host sides of the kernels that generate
// them (srs_host.cpp, pusch_chest_host.cpp): N_zc and the Zadoff-Chu root q of the sizes M_zc >= 36, in the reference's
// arithmetic (low_papr_sequence_generator_impl.cpp:134-156).
#pragma once

#include "nrphy_host_internal.h"

#pragma GCC visibility push(hidden)

// prime_lower_than: the largest prime below n (n >= 36 here).
inline uint32_t low_papr_prime_below(uint32_t n)
{
  for (uint32_t v = n - 1; v > 2; --v) {
    bool prime = true;
    for (uint32_t f = 2; f * f <= v; ++f) {
      if (v % f == 0) {
        prime = false;
        break;
      }
    }
    if (prime) {
      return v;
    }
  }
  return 2;
}

// zc_sequence_q(u, 0, N_zc): single precision, the half added in double.
inline uint32_t low_papr_zc_root(uint32_t u, uint32_t n_zc)
{
  const float n_sz  = (float)n_zc;
  const float q_hat = n_sz * (float)(u + 1) / 31;
  const float q     = (float)((double)q_hat + 0.5);
  return (uint32_t)(int)q;
}

#pragma GCC visibility pop
