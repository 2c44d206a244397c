// CSI part 2 of a PUSCH, the device-free part: the checks of a size description (uci_part2_size_description), its evaluation
// on a CSI part 1 payload (uci_part2_get_size, R/lib/ran/uci/uci_part2_size_calculator.cpp) and the enumeration of every size a
// description can give -- what the processor's plan (pusch_csi2_host.cpp) derives its variants from.  No HIP, no device: only the
// public header, so that tests/pusch_csi2_check.cpp compiles it alone.
//
// A parameter's value is `width` payload bits from `offset` on with the payload bit at `offset` as its MOST significant bit: the
// reference reads the slice into a word with that bit lowest (bounded_bitset::to_uint64) and then reverses the word's bits.  A
// recording of the reference's processor pins this (tests/golden/record_pusch_csi2_reference.cpp).  An entry's index is the
// concatenation of its parameters, the first one in the high bits; the size is the sum of map[index] over the entries.
#pragma once

#include "mi355_nrphy.h"

#include <algorithm>
#include <cstdint>

constexpr uint32_t PUSCH_CSI2_MAX_UCI_BITS = 1706; // what nrphy_ul_sch_info takes for a UCI part

// Sum of an entry's widths, or -1 for an entry the description may not hold.
inline int pusch_csi2_entry_bits(const nrphy_pusch_csi2_entry_t& e, uint32_t nof_csi_part1)
{
  if (e.nof_parameters > NRPHY_PUSCH_CSI2_MAX_PARAMETERS) {
    return -1;
  }
  uint32_t bits = 0;
  for (uint32_t k = 0; k != e.nof_parameters; ++k) {
    if (e.width[k] > NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS || e.offset[k] > nof_csi_part1 || e.width[k] > nof_csi_part1 - e.offset[k]) {
      return -1;
    }
    bits += e.width[k];
  }
  if (bits > NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS || e.map_size != (1U << bits)) {
    return -1;
  }
  return (int)bits;
}

// The structure of a description with at least one entry against a CSI part 1 of nof_csi_part1 bits.
inline bool pusch_csi2_desc_ok(const nrphy_pusch_csi2_desc_t& d, uint32_t nof_csi_part1)
{
  if (d.nof_entries == 0 || d.nof_entries > NRPHY_PUSCH_CSI2_MAX_ENTRIES || nof_csi_part1 == 0) {
    return false;
  }
  for (uint32_t i = 0; i != d.nof_entries; ++i) {
    if (pusch_csi2_entry_bits(d.entries[i], nof_csi_part1) < 0) {
      return false;
    }
  }
  return true;
}

// The index of one entry for a payload of one bit per byte (only bit 0 of a byte counts).
inline uint32_t pusch_csi2_entry_index(const nrphy_pusch_csi2_entry_t& e, const uint8_t* csi_part1_bits)
{
  uint32_t index = 0;
  for (uint32_t k = 0; k != e.nof_parameters; ++k) {
    uint32_t value = 0;
    for (uint32_t j = 0; j != e.width[k]; ++j) {
      value |= (uint32_t)(csi_part1_bits[e.offset[k] + j] & 1U) << (e.width[k] - 1 - j);
    }
    index = (index << e.width[k]) | value;
  }
  return index;
}

// uci_part2_get_size for a description pusch_csi2_desc_ok accepts.
inline uint32_t pusch_csi2_size(const nrphy_pusch_csi2_desc_t& d, const uint8_t* csi_part1_bits)
{
  uint32_t size = 0;
  for (uint32_t i = 0; i != d.nof_entries; ++i) {
    size += d.entries[i].map[pusch_csi2_entry_index(d.entries[i], csi_part1_bits)];
  }
  return size;
}

// Every size the description can give: sizes[0] = 0 ("no part 2"), then the distinct non-zero sums of one map value per entry in
// ascending order; *nof_variants counts them all.  False for a map value or a sum above PUSCH_CSI2_MAX_UCI_BITS and for more than
// NRPHY_PUSCH_CSI2_MAX_SIZES distinct non-zero sums.  sizes has room for NRPHY_PUSCH_CSI2_MAX_VARIANTS.
inline bool pusch_csi2_enumerate(const nrphy_pusch_csi2_desc_t& d, uint32_t* nof_variants, uint32_t* sizes)
{
  uint32_t n = 1;
  sizes[0]   = 0;
  const nrphy_pusch_csi2_entry_t& e0     = d.entries[0];
  const bool                      two    = d.nof_entries > 1;
  const uint32_t                  n_last = two ? d.entries[1].map_size : 1;
  for (uint32_t a = 0; a != e0.map_size; ++a) {
    for (uint32_t b = 0; b != n_last; ++b) {
      const uint32_t second = two ? d.entries[1].map[b] : 0;
      if (e0.map[a] > PUSCH_CSI2_MAX_UCI_BITS || second > PUSCH_CSI2_MAX_UCI_BITS || e0.map[a] + second > PUSCH_CSI2_MAX_UCI_BITS) {
        return false;
      }
      const uint32_t size = e0.map[a] + second;
      if (std::find(sizes, sizes + n, size) != sizes + n) {
        continue;
      }
      if (n == NRPHY_PUSCH_CSI2_MAX_VARIANTS) {
        return false;
      }
      sizes[n++] = size;
    }
  }
  std::sort(sizes, sizes + n);
  *nof_variants = n;
  return true;
}
