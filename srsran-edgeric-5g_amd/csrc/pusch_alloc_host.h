// What the host sides of the receive-side PUSCH steps share (pusch_demod_host.cpp, pusch_chest_host.cpp): "a PUSCH on a received
// grid" -- the allocation's fields common to their descriptors, the checks of the allocation against the grid, and its list of
// PRBs.  What a step requires beyond that stays in its own file.
#pragma once

#include "nrphy_host_internal.h"

#pragma GCC visibility push(hidden)

constexpr uint32_t MAX_PRB_BITS = NRPHY_PRB_WORDS * 64;

// The allocation fields of nrphy_pusch_demod_cfg_t / nrphy_pusch_chest_cfg_t (same names and types in both).
struct PuschAllocation {
  const uint64_t* prb_mask; // [NRPHY_PRB_WORDS]
  uint32_t        start_symbol_index, nof_symbols, dmrs_symbol_mask, nof_rx_ports;
  const uint32_t* rx_ports; // [NRPHY_MAX_PORTS]
};
template <class Cfg>
inline PuschAllocation pusch_allocation(const Cfg& c)
{
  return {c.prb_mask, c.start_symbol_index, c.nof_symbols, c.dmrs_symbol_mask, c.nof_rx_ports, c.rx_ports};
}

inline uint32_t nof_prb(const PuschAllocation& a)
{
  uint32_t n = 0;
  for (uint32_t w = 0; w != NRPHY_PRB_WORDS; ++w) {
    n += (uint32_t)__builtin_popcountll(a.prb_mask[w]);
  }
  return n;
}

// The grid's dimensions; 1 to NRPHY_MAX_PORTS distinct receive ports, each a port of the grid; no PRB beyond the grid; the
// symbols inside the slot.
inline bool allocation_fits_grid(const PuschAllocation& a, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  if (grid_nof_subc == 0 || grid_nof_subc % NRPHY_NRE != 0 || grid_nof_subc > NRPHY_MAX_RB * NRPHY_NRE || grid_nof_ports == 0 ||
      grid_nof_ports > NRPHY_MAX_PORTS || a.nof_rx_ports < 1 || a.nof_rx_ports > NRPHY_MAX_PORTS) {
    return false;
  }
  for (uint32_t i = 0; i != a.nof_rx_ports; ++i) {
    if (a.rx_ports[i] >= grid_nof_ports) {
      return false;
    }
    for (uint32_t j = 0; j != i; ++j) {
      if (a.rx_ports[j] == a.rx_ports[i]) {
        return false;
      }
    }
  }
  for (uint32_t b = grid_nof_subc / NRPHY_NRE; b != MAX_PRB_BITS; ++b) {
    if ((a.prb_mask[b / 64] >> (b % 64)) & 1U) {
      return false;
    }
  }
  return a.start_symbol_index < NRPHY_NSYMB && a.nof_symbols <= NRPHY_NSYMB - a.start_symbol_index;
}

// Appends the allocated PRBs (grid-indexed, ascending) to a plan's list; returns how many.
inline uint32_t append_prbs(const PuschAllocation& a, uint32_t grid_nof_subc, std::vector<uint16_t>& prbs)
{
  const size_t first = prbs.size();
  for (uint32_t b = 0; b != grid_nof_subc / NRPHY_NRE; ++b) {
    if ((a.prb_mask[b / 64] >> (b % 64)) & 1U) {
      prbs.push_back((uint16_t)b);
    }
  }
  return (uint32_t)(prbs.size() - first);
}

#pragma GCC visibility pop
