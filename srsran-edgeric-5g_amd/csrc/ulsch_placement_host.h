// Where the soft bits of a PUSCH codeword with UCI go (TS 38.212 Section 6.2.7): the placement ulsch_demultiplex_impl computes
// symbol by symbol (configure_current_ofdm_symbol, configure_csi_part2_current_ofdm_symbol and re_set_select of
// R/lib/phy/upper/channel_processors/pusch/ulsch_demultiplex_impl.cpp:74-96,331-472), computed once per plan for the whole
// codeword.  Resource elements are counted as the demodulator delivers them: the data REs of the allocation symbol by symbol,
// subcarrier ascending, nof_layers * Qm soft bits each.
#pragma once

#include "nrphy_host_internal.h"

#include <vector>

#pragma GCC visibility push(hidden)

enum UlschStream : uint32_t { ULSCH_SCH = 0, ULSCH_HARQ = 1, ULSCH_CSI1 = 2, ULSCH_CSI2 = 3 };
enum UlschFix : uint32_t { ULSCH_FIX_NONE = 0, ULSCH_FIX_1BIT = 1, ULSCH_FIX_2BIT = 2 };
constexpr uint32_t ULSCH_MAP_ZERO = nrphy::ULSCH_MAP_ZERO_BIT, ULSCH_MAP_SKIP = nrphy::ULSCH_MAP_SKIP_BIT,
                   ULSCH_MAP_INDEX = nrphy::ULSCH_MAP_INDEX_MASK; // the map entry's layout: nrphy_internal.h

struct UlschSpecial { // an RE that needs more than a copy: src RE of the codeword -> RE dst of `stream`, with a correction
  uint32_t src, dst, stream, fix;
};

struct UlschPlacement {
  uint32_t                  bits_per_re = 0;
  uint32_t                  nof_re[4]   = {0, 0, 0, 0}; // REs per output stream
  std::vector<uint32_t>     map;                        // per input RE
  std::vector<UlschSpecial> special;
};

inline bool ulsch_bits_per_symbol(uint32_t modulation, uint32_t* bps)
{
  switch (modulation) {
    case NRPHY_MOD_PI2_BPSK:
    case NRPHY_MOD_BPSK:
      *bps = 1;
      return true;
    case NRPHY_MOD_QPSK:
    case NRPHY_MOD_QAM16:
    case NRPHY_MOD_QAM64:
    case NRPHY_MOD_QAM256:
      *bps = modulation;
      return true;
    default:
      return false;
  }
}

// re_set_select: of the candidates (ascending) every d-th, `count` of them.
inline void ulsch_select(const std::vector<uint32_t>& candidates, uint32_t d, uint32_t count, std::vector<uint32_t>& out)
{
  out.clear();
  for (uint32_t i = 0; i != count; ++i) {
    out.push_back(candidates[(size_t)i * d]);
  }
}

// false for what the reference asserts on, see nrphy_ulsch_demux_validate.
inline bool ulsch_placement(const nrphy_ulsch_demux_cfg_t& c, UlschPlacement& p)
{
  uint32_t qm = 0;
  if (!ulsch_bits_per_symbol(c.modulation, &qm) || c.nof_layers < 1 || c.nof_layers > NRPHY_MAX_PORTS || c.nof_prb < 1 ||
      c.nof_prb > NRPHY_MAX_RB || c.nof_symbols < 1 || c.start_symbol_index >= NRPHY_NSYMB ||
      c.nof_symbols > NRPHY_NSYMB - c.start_symbol_index || c.dmrs_type > 1 || c.nof_cdm_groups_without_data < 1 ||
      c.nof_cdm_groups_without_data > (c.dmrs_type == 0 ? 2U : 3U) || (c.dmrs_symbol_mask >> NRPHY_NSYMB) != 0) {
    return false;
  }
  // A payload without soft bits or soft bits without a payload; a reserved set next to HARQ-ACK of more than 2 bits.
  if ((c.nof_harq_ack_bits == 0) != (c.nof_enc_harq_ack_bits == 0) || (c.nof_csi_part1_bits == 0) != (c.nof_enc_csi_part1_bits == 0) ||
      (c.nof_csi_part2_bits == 0) != (c.nof_enc_csi_part2_bits == 0) || (c.nof_harq_ack_bits > 2 && c.nof_harq_ack_rvd != 0)) {
    return false;
  }
  // l1: the first symbol without DM-RS after the first with; l1_csi: the first symbol without DM-RS.
  uint32_t first_dmrs = 0;
  while (first_dmrs != NRPHY_NSYMB && !((c.dmrs_symbol_mask >> first_dmrs) & 1U)) {
    ++first_dmrs;
  }
  uint32_t l1 = first_dmrs;
  while (l1 < NRPHY_NSYMB && ((c.dmrs_symbol_mask >> l1) & 1U)) {
    ++l1;
  }
  uint32_t l1_csi = 0;
  while (l1_csi != NRPHY_NSYMB && ((c.dmrs_symbol_mask >> l1_csi) & 1U)) {
    ++l1_csi;
  }
  if (first_dmrs == NRPHY_NSYMB || l1 >= NRPHY_NSYMB || l1_csi == NRPHY_NSYMB) {
    return false;
  }
  const uint32_t nbre        = qm * c.nof_layers;
  const uint32_t re_dmrs     = (NRPHY_NRE - c.nof_cdm_groups_without_data * (c.dmrs_type == 0 ? 6U : 4U)) * c.nof_prb;
  const uint32_t harq_fix    = qm == 1 ? ULSCH_FIX_NONE : c.nof_harq_ack_bits == 1 ? ULSCH_FIX_1BIT : ULSCH_FIX_2BIT;
  const uint32_t part_bits[4] = {0, c.nof_harq_ack_bits, c.nof_csi_part1_bits, c.nof_csi_part2_bits};
  p                          = UlschPlacement();
  p.bits_per_re              = nbre;
  uint32_t m_rvd = 0, m_harq = 0, m_csi1 = 0, m_csi2 = 0;
  std::vector<uint32_t> cand, rvd, sel;
  std::vector<uint8_t>  owner, is_rvd, punctured; // per RE of the symbol
  for (uint32_t l = c.start_symbol_index; l != c.start_symbol_index + c.nof_symbols; ++l) {
    const bool     dmrs = (c.dmrs_symbol_mask >> l) & 1U;
    const uint32_t M    = dmrs ? re_dmrs : c.nof_prb * NRPHY_NRE;
    owner.assign(M, ULSCH_SCH);
    is_rvd.assign(M, 0);
    punctured.assign(M, 0);
    uint32_t M_uci = dmrs ? 0 : M, M_rvd = 0;
    auto stride = [](uint32_t available, uint32_t remainder, uint32_t* d, uint32_t* count) {
      *d     = remainder < available ? available / remainder : 1;
      *count = remainder < available ? remainder : available;
    };
    auto candidates = [&](bool without_rvd) { // the REs still free for UCI, ascending
      cand.clear();
      for (uint32_t i = 0; i != (dmrs ? 0 : M); ++i) {
        if (owner[i] == ULSCH_SCH && !(without_rvd && is_rvd[i])) {
          cand.push_back(i);
        }
      }
    };
    auto take = [&](uint32_t stream) {
      for (uint32_t i : sel) {
        owner[i] = (uint8_t)stream;
      }
    };
    uint32_t d = 1, count = 0;
    // Step 1: the reserved set.
    const uint32_t rem_rvd = (c.nof_harq_ack_rvd - m_rvd) / nbre;
    if (c.nof_harq_ack_rvd >= m_rvd && l >= l1 && M_uci > 0 && rem_rvd > 0) {
      stride(M_uci, rem_rvd, &d, &count);
      candidates(false);
      ulsch_select(cand, d, count, rvd);
      for (uint32_t i : rvd) {
        is_rvd[i] = 1;
      }
      M_rvd = count;
      m_rvd += count * nbre;
    }
    // Step 2: HARQ-ACK of more than 2 bits.
    const uint32_t rem_harq = (c.nof_enc_harq_ack_bits - m_harq) / nbre;
    if (l >= l1 && M_uci > 0 && c.nof_harq_ack_bits > 2 && rem_harq > 0) {
      stride(M_uci, rem_harq, &d, &count);
      candidates(false);
      ulsch_select(cand, d, count, sel);
      take(ULSCH_HARQ);
      M_uci -= count;
      m_harq += count * nbre;
    }
    // Step 3: CSI part 1 outside the reserved set.
    const uint32_t rem_csi1 = (c.nof_enc_csi_part1_bits - m_csi1) / nbre;
    if (l >= l1_csi && M_uci > M_rvd && rem_csi1 > 0) {
      stride(M_uci - M_rvd, rem_csi1, &d, &count);
      candidates(true);
      ulsch_select(cand, d, count, sel);
      take(ULSCH_CSI1);
      M_uci -= count;
      m_csi1 += count * nbre;
    }
    // Step 3bis: CSI part 2, reserved REs included.
    const uint32_t rem_csi2 = (c.nof_enc_csi_part2_bits - m_csi2) / nbre;
    if (l >= l1_csi && M_uci > 0 && rem_csi2 > 0) {
      stride(M_uci, rem_csi2, &d, &count);
      candidates(false);
      ulsch_select(cand, d, count, sel);
      take(ULSCH_CSI2);
      m_csi2 += count * nbre;
    }
    // Step 5: HARQ-ACK of 1 or 2 bits punctures the reserved set.
    if (M_rvd > 0 && c.nof_harq_ack_bits <= 2 && rem_harq > 0) {
      stride(M_rvd, rem_harq, &d, &count);
      ulsch_select(rvd, d, count, sel);
      for (uint32_t i : sel) {
        punctured[i] = 1;
      }
      m_harq += count * nbre;
    }
    // The symbol's REs in the order the reference hands them on: every stream ascending.
    const uint32_t base = (uint32_t)p.map.size();
    p.map.resize(base + M);
    for (uint32_t i = 0; i != M; ++i) {
      if (punctured[i]) {
        p.special.push_back({base + i, p.nof_re[ULSCH_HARQ]++, ULSCH_HARQ, harq_fix});
      }
    }
    for (uint32_t i = 0; i != M; ++i) {
      const uint32_t s     = owner[i];
      const uint32_t dst   = p.nof_re[s]++;
      uint32_t       entry = (s << 29) | dst;
      if (punctured[i]) {
        entry |= ULSCH_MAP_ZERO;
      } else if (s != ULSCH_SCH && qm != 1 && (part_bits[s] == 1 || part_bits[s] == 2)) {
        entry |= ULSCH_MAP_SKIP;
        p.special.push_back({base + i, dst, s, part_bits[s] == 1 ? (uint32_t)ULSCH_FIX_1BIT : (uint32_t)ULSCH_FIX_2BIT});
      }
      p.map[base + i] = entry;
    }
  }
  // on_end_codeword: every UCI soft bit must have been taken.
  return m_harq == c.nof_enc_harq_ack_bits && m_csi1 == c.nof_enc_csi_part1_bits && m_csi2 == c.nof_enc_csi_part2_bits &&
         p.map.size() <= ULSCH_MAP_INDEX;
}

#pragma GCC visibility pop
