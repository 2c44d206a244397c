// The UL-SCH / UCI rate-matching sizes of a PUSCH (TS 38.212 Section 6.3.2.4): what get_ulsch_information
// (R/lib/ran/pusch/ulsch_info.cpp:30-360) derives from the transport-block size, the UCI payload sizes, alpha and the beta
// offsets -- the segmentation of get_sch_segmentation_info (R/lib/ran/sch/sch_segmentation.cpp:30-63), Q'_ACK, the reserved set,
// Q'_CSI-1, Q'_CSI-2 and the soft bits left to the UL-SCH.  Pure host arithmetic, no device.
//
// The float expressions keep the reference's order of operations: (O + L) * beta * N_RE / sum K_r for a PUSCH with UL-SCH,
// (O + L) * beta / (R * Qm) for one without, ceil(alpha * N_RE) for the caps.  Where the reference's unsigned arithmetic would
// wrap (a cap below what HARQ-ACK already took, more UCI RE than the allocation has) the configuration is refused instead.
#pragma once

#include "nrphy_host_internal.h"

#include <cmath>

#pragma GCC visibility push(hidden)

// get_uci_crc_size
inline uint32_t ulsch_info_uci_crc_bits(uint32_t payload_bits)
{
  return payload_bits < 12 ? 0 : payload_bits < 20 ? 6 : 11;
}

// ceil of a float as an unsigned count; false where the conversion the reference makes is not defined (negative, NaN, 2^31 or more).
inline bool ulsch_info_ceil(float v, uint32_t* out)
{
  const float c = std::ceil(v);
  if (!(c >= 0.0F) || !(c < 2147483648.0F)) {
    return false;
  }
  *out = (uint32_t)c;
  return true;
}

// calculate_nof_re_harq_ack and calculate_nof_re_harq_ack_without_sch: min(left, ceil(alpha * N_RE,l0)).
inline bool ulsch_info_re_harq_ack(const nrphy_ulsch_info_cfg_t& c, uint32_t nof_bits, bool with_sch, float rate, uint32_t qm,
                                   uint32_t nof_re_uci, uint32_t sum_cb_bits, uint32_t nof_re_uci_l0, uint32_t* out)
{
  *out = 0;
  if (nof_bits == 0) {
    return true;
  }
  const float payload = (float)(nof_bits + ulsch_info_uci_crc_bits(nof_bits));
  uint32_t    left = 0, right = 0;
  if (!ulsch_info_ceil(with_sch ? payload * c.beta_offset_harq_ack * (float)nof_re_uci / (float)sum_cb_bits
                                : payload * c.beta_offset_harq_ack / (rate * (float)qm),
                       &left) ||
      !ulsch_info_ceil(c.alpha_scaling * (float)nof_re_uci_l0, &right)) {
    return false;
  }
  *out = std::min(left, right);
  return true;
}

// NRPHY_OK and *out filled, or NRPHY_ERR_ARGUMENT: see nrphy_ul_sch_info in include/mi355_nrphy.h.
inline int ulsch_info(const nrphy_ulsch_info_cfg_t& c, nrphy_ulsch_info_t& out)
{
  std::memset(&out, 0, sizeof(out));
  uint32_t qm = 0;
  switch (c.modulation) {
    case NRPHY_MOD_PI2_BPSK:
    case NRPHY_MOD_BPSK:
      qm = 1;
      break;
    case NRPHY_MOD_QPSK:
    case NRPHY_MOD_QAM16:
    case NRPHY_MOD_QAM64:
    case NRPHY_MOD_QAM256:
      qm = c.modulation;
      break;
    default:
      return NRPHY_ERR_ARGUMENT;
  }
  const float rate = c.target_code_rate * (1.F / 1024); // sch_mcs_description::get_normalised_target_code_rate
  if (!(rate > 0.F && rate < 1.F) || !std::isfinite(c.alpha_scaling) || !(c.alpha_scaling >= 0.F) ||
      !std::isfinite(c.beta_offset_harq_ack) || !(c.beta_offset_harq_ack >= 0.F) || !std::isfinite(c.beta_offset_csi_part1) ||
      !(c.beta_offset_csi_part1 >= 0.F) || !std::isfinite(c.beta_offset_csi_part2) || !(c.beta_offset_csi_part2 >= 0.F)) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The reference's assertions on the allocation.
  if ((c.dmrs_type != 1 && c.dmrs_type != 2) || c.nof_cdm_groups_without_data < 1 ||
      c.nof_cdm_groups_without_data > (c.dmrs_type == 1 ? 2U : 3U) || c.nof_rb == 0 || c.nof_rb > NRPHY_MAX_RB || c.nof_layers == 0 ||
      c.nof_layers > NRPHY_MAX_LAYERS || c.nof_symbols == 0 || c.start_symbol_index >= NRPHY_NSYMB ||
      c.nof_symbols > NRPHY_NSYMB - c.start_symbol_index || c.contains_dc > 1 || c.nof_harq_ack_bits > 1706 ||
      c.nof_csi_part1_bits > 1706 || c.nof_csi_part2_bits > 1706 || c.tbs_bits > 8U * NRPHY_MAX_TB_BYTES) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t inside = ((1U << c.nof_symbols) - 1U) << c.start_symbol_index;
  if (c.dmrs_symbol_mask == 0 || (c.dmrs_symbol_mask & ~inside) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  const bool with_sch = c.tbs_bits > 0;
  uint32_t   sum_cb_bits = 0;
  if (with_sch) {
    const uint32_t tb_crc = c.tbs_bits <= 3824 ? 16 : 24;
    const uint32_t b      = c.tbs_bits + tb_crc;
    const uint32_t bg     = (c.tbs_bits <= 292 || rate <= 0.25F || (c.tbs_bits <= 3824 && rate <= 0.67F)) ? 2 : 1; // get_ldpc_base_graph
    const uint32_t kcb    = bg == 1 ? 8448 : 3840;
    const uint32_t ncb    = b <= kcb ? 1 : divide_ceil(b, kcb - 24);
    uint32_t       ref_len = 22;
    if (bg == 2) {
      ref_len = b > 640 ? 10 : b > 560 ? 9 : b > 192 ? 8 : 6;
    }
    const uint32_t b_out = b + (ncb > 1 ? 24 * ncb : 0);
    uint32_t       zc    = 0;
    for (uint32_t i = 0; i != NOF_LIFTING_SIZES; ++i) {
      if (LIFTING_SIZES[i] * ncb * ref_len >= b_out) {
        zc = LIFTING_SIZES[i];
        break;
      }
    }
    if (zc == 0) {
      return NRPHY_ERR_ARGUMENT;
    }
    out.has_sch                = 1;
    out.tb_crc_bits            = tb_crc;
    out.base_graph             = bg;
    out.nof_cb                 = ncb;
    out.lifting_size           = zc;
    out.nof_bits_per_cb        = (bg == 1 ? 22 : 10) * zc;
    out.nof_filler_bits_per_cb = out.nof_bits_per_cb - (b / ncb + (ncb > 1 ? 24 : 0));
    sum_cb_bits                = ncb * out.nof_bits_per_cb;
  }
  const uint32_t nof_symbols_dmrs   = (uint32_t)__builtin_popcount(c.dmrs_symbol_mask);
  const uint32_t nof_re_dmrs_per_rb = nof_symbols_dmrs * c.nof_cdm_groups_without_data * (c.dmrs_type == 1 ? 6U : 4U);
  const uint32_t nof_re_total       = c.nof_rb * (c.nof_symbols * NRPHY_NRE - nof_re_dmrs_per_rb);
  const uint32_t nof_re_uci         = (c.nof_symbols - nof_symbols_dmrs) * c.nof_rb * NRPHY_NRE;
  // RE that can carry UCI from the first DM-RS symbol on.
  uint32_t nof_re_uci_l0 = 0;
  for (uint32_t l = (uint32_t)__builtin_ctz(c.dmrs_symbol_mask); l != c.start_symbol_index + c.nof_symbols; ++l) {
    if (((c.dmrs_symbol_mask >> l) & 1U) == 0) {
      nof_re_uci_l0 += c.nof_rb * NRPHY_NRE;
    }
  }
  uint32_t alpha_cap = 0; // ceil(alpha * N_RE): the right-hand sides of CSI part 1 and part 2 with UL-SCH
  if (!ulsch_info_ceil(c.alpha_scaling * (float)nof_re_uci, &alpha_cap)) {
    return NRPHY_ERR_ARGUMENT;
  }

  if (!ulsch_info_re_harq_ack(c, c.nof_harq_ack_bits, with_sch, rate, qm, nof_re_uci, sum_cb_bits, nof_re_uci_l0, &out.nof_harq_ack_re)) {
    return NRPHY_ERR_ARGUMENT;
  }
  // Up to two HARQ-ACK bits: the reserved set, sized as for two bits.
  uint32_t nof_harq_ack_rvd_re = 0;
  if (c.nof_harq_ack_bits < 2) {
    if (!ulsch_info_re_harq_ack(c, 2, with_sch, rate, qm, nof_re_uci, sum_cb_bits, nof_re_uci_l0, &nof_harq_ack_rvd_re)) {
      return NRPHY_ERR_ARGUMENT;
    }
  } else if (c.nof_harq_ack_bits == 2) {
    nof_harq_ack_rvd_re = out.nof_harq_ack_re;
  }
  const uint32_t harq_re_csi1 = c.nof_harq_ack_bits <= 2 ? nof_harq_ack_rvd_re : out.nof_harq_ack_re;
  const uint32_t harq_re_csi2 = c.nof_harq_ack_bits <= 2 ? 0 : out.nof_harq_ack_re;

  // CSI part 1.
  if (c.nof_csi_part1_bits != 0) {
    const float payload = (float)(c.nof_csi_part1_bits + ulsch_info_uci_crc_bits(c.nof_csi_part1_bits));
    uint32_t    left    = 0;
    if (with_sch) {
      if (!ulsch_info_ceil(payload * c.beta_offset_csi_part1 * (float)nof_re_uci / (float)sum_cb_bits, &left) || alpha_cap < harq_re_csi1) {
        return NRPHY_ERR_ARGUMENT;
      }
      out.nof_csi_part1_re = std::min(left, alpha_cap - harq_re_csi1);
    } else {
      if (nof_re_uci < harq_re_csi1) {
        return NRPHY_ERR_ARGUMENT;
      }
      out.nof_csi_part1_re = nof_re_uci - harq_re_csi1;
      if (c.nof_csi_part2_bits != 0) {
        if (!ulsch_info_ceil(payload * c.beta_offset_csi_part1 / (rate * (float)qm), &left)) {
          return NRPHY_ERR_ARGUMENT;
        }
        out.nof_csi_part1_re = std::min(left, out.nof_csi_part1_re);
      }
    }
  }
  // CSI part 2.
  if (c.nof_csi_part2_bits != 0) {
    const uint32_t taken = harq_re_csi2 + out.nof_csi_part1_re;
    if (with_sch) {
      const float payload = (float)(c.nof_csi_part2_bits + ulsch_info_uci_crc_bits(c.nof_csi_part2_bits));
      uint32_t    left    = 0;
      if (!ulsch_info_ceil(payload * c.beta_offset_csi_part2 * (float)nof_re_uci / (float)sum_cb_bits, &left) || alpha_cap < taken) {
        return NRPHY_ERR_ARGUMENT;
      }
      out.nof_csi_part2_re = std::min(left, alpha_cap - taken);
    } else {
      if (nof_re_uci < taken) {
        return NRPHY_ERR_ARGUMENT;
      }
      out.nof_csi_part2_re = nof_re_uci - taken;
    }
  }
  // UL-SCH: what HARQ-ACK of more than two bits and the CSI parts leave.
  uint32_t nof_re_ul_sch = 0;
  if (with_sch) {
    const uint32_t uci_re = (c.nof_harq_ack_bits > 2 ? out.nof_harq_ack_re : 0) + out.nof_csi_part1_re + out.nof_csi_part2_re;
    if (nof_re_total < uci_re) {
      return NRPHY_ERR_ARGUMENT;
    }
    nof_re_ul_sch = nof_re_total - uci_re;
  }
  const uint32_t bits_per_re = c.nof_layers * qm;
  out.nof_ul_sch_bits        = nof_re_ul_sch * bits_per_re;
  out.nof_harq_ack_bits      = out.nof_harq_ack_re * bits_per_re;
  out.nof_harq_ack_rvd       = nof_harq_ack_rvd_re * bits_per_re;
  out.nof_csi_part1_bits     = out.nof_csi_part1_re * bits_per_re;
  out.nof_csi_part2_bits     = out.nof_csi_part2_re * bits_per_re;
  out.nof_dc_overlap_bits    = c.contains_dc ? c.nof_symbols * qm : 0;
  return NRPHY_OK;
}

#pragma GCC visibility pop
