// Plan-time constants of port_channel_estimator_average_impl shared by the host sides of the kernels that run it
// (pusch_chest_host.cpp, pucch_host.cpp, pucch2_host.cpp): the raised-cosine table and the taps resampled from it (filter_type,
// port_channel_estimator_average_impl.cpp:41-47,62-111), the number of virtual pilots (apply_fd_smoothing, :621-625) and the
// symbol start epochs (initialize_symbol_start_epochs, :454-466), in float32 and in the reference's order of operations.
#pragma once

#include "nrphy_host_internal.h"

#pragma GCC visibility push(hidden)

constexpr float CHEST_RC_FILTER[31] = {-0.0641253f, -0.0660711f, -0.0611526f, -0.0485918f, -0.0281126f, 0.0000000f, 0.0348830f, 0.0751249f,
                                       0.1188406f,  0.1637874f,  0.2075139f,  0.2475302f,  0.2814857f,  0.3073415f, 0.3235207f, 0.3290274f,
                                       0.3235207f,  0.3073415f,  0.2814857f,  0.2475302f,  0.2075139f,  0.1637874f, 0.1188406f, 0.0751249f,
                                       0.0348830f,  0.0000000f,  -0.0281126f, -0.0485918f, -0.0611526f, -0.0660711f, -0.0641253f};

// filter_type(nof_rb, stride): taps resampled from the table and normalised, in float as the reference does.  Pilots on every
// `stride`-th subcarrier: 2 for the PUSCH DM-RS (5, 11 or 15 taps), 3 for PUCCH format 2 (3, 7 or 11).
inline uint32_t chest_filter_taps(uint32_t nof_rb, uint32_t stride, float* taps)
{
  nof_rb           = std::min(nof_rb, 3U);
  uint32_t nof_out = (nof_rb * 10 + 1) / 2 / stride;
  uint32_t n       = 31 / 2 - nof_out * stride;
  nof_out          = 2 * nof_out + 1;
  float total      = 0;
  for (uint32_t i = 0; i != nof_out; ++i) {
    taps[i] = CHEST_RC_FILTER[n];
    total += taps[i];
    n += stride;
  }
  const float rcp = 1 / total;
  for (uint32_t i = 0; i != nof_out; ++i) {
    taps[i] = taps[i] * rcp;
  }
  return nof_out;
}

// Virtual pilots per side: every pilot of a single PRB, else half the filter, at most 12.
inline uint32_t chest_nof_virtual_pilots(uint32_t nof_rb, uint32_t pilots_per_rb, uint32_t ntaps)
{
  return nof_rb == 1 ? pilots_per_rb : std::min(12U, ntaps / 2);
}

// Start of every symbol of the slot in symbols, normal cyclic prefix: cyclic prefix lengths in units of kappa
// (cyclic_prefix::get_length) as fractions of a symbol, accumulated.
inline void chest_symbol_epochs(uint32_t numerology, float (&epoch)[NRPHY_NSYMB])
{
  double e = 0;
  for (uint32_t l = 0; l != NRPHY_NSYMB; ++l) {
    const uint32_t cp = (144U >> numerology) + ((l == 0 || l == 7U * (1U << numerology)) ? 16U : 0U);
    e += (double)cp * (double)(1U << numerology) / 2048.0 + (l == 0 ? 0.0 : 1.0);
    epoch[l] = (float)e;
  }
}

#pragma GCC visibility pop
