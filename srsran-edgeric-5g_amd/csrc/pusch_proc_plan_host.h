// The PUSCH processor's plan (pusch_proc_host.cpp) and the steps of its run, for the processor with CSI part 2
// (pusch_csi2_host.cpp), which owns such a plan and runs its own launches between those steps.  Not part of the ABI.
#pragma once

#include "nrphy_host_internal.h"

#include <vector>

#pragma GCC visibility push(hidden) // internal to the library

struct ProcDecoder {
  nrphy_pusch_decoder_cfg_t cfg;
  uint32_t                  pdu;
  uint64_t                  llr_offset; // into the UL-SCH stream buffer (with UCI) or the codeword buffer (without)
  bool                      from_sch;
  uint64_t                  soft_offset, state_offset, tb_offset;
};

// The ulsch_configuration of a PDU over nof_rb PRBs with a CSI part 2 of nof_csi_part2_bits (pusch_processor_impl.cpp:138-164).
inline nrphy_ulsch_info_cfg_t pusch_proc_info_cfg(const nrphy_pusch_pdu_t& p, uint32_t nof_rb, uint32_t nof_csi_part2_bits)
{
  nrphy_ulsch_info_cfg_t ic;
  std::memset(&ic, 0, sizeof(ic));
  ic.tbs_bits                    = 8 * p.tb_size_bytes;
  ic.modulation                  = p.modulation;
  ic.target_code_rate            = p.target_code_rate;
  ic.nof_harq_ack_bits           = p.nof_harq_ack;
  ic.nof_csi_part1_bits          = p.nof_csi_part1;
  ic.nof_csi_part2_bits          = nof_csi_part2_bits;
  ic.alpha_scaling               = p.alpha_scaling;
  ic.beta_offset_harq_ack        = p.beta_offset_harq_ack;
  ic.beta_offset_csi_part1       = p.beta_offset_csi_part1;
  ic.beta_offset_csi_part2       = p.beta_offset_csi_part2;
  ic.nof_rb                      = nof_rb;
  ic.start_symbol_index          = p.start_symbol_index;
  ic.nof_symbols                 = p.nof_symbols;
  ic.dmrs_type                   = p.dmrs_type;
  ic.dmrs_symbol_mask            = p.dmrs_symbol_mask;
  ic.nof_cdm_groups_without_data = p.nof_cdm_groups_without_data;
  ic.nof_layers                  = p.nof_tx_layers;
  ic.contains_dc = (p.dc_position != NRPHY_PUSCH_CHEST_NO_DC && mask_test(p.prb_mask, p.dc_position / NRPHY_NRE)) ? 1 : 0;
  return ic;
}

#pragma GCC visibility pop

struct nrphy_pusch_proc_plan {
  nrphy_ctx*                 ctx = nullptr;
  uint32_t                   n   = 0;
  nrphy_pusch_chest_plan_t*  chest = nullptr;
  nrphy_pusch_demod_plan_t*  demod = nullptr;
  nrphy_ulsch_demux_plan_t*  demux = nullptr;
  nrphy_uci_decoder_plan_t*  uci   = nullptr;
  std::vector<ProcDecoder>   decoders;
  std::vector<uint64_t>      soft_bytes, state_bytes; // per PDU
  std::vector<PuschProcDesc> desc;                    // the host's copy of d_desc
  uint64_t                   llr_stride = 0;
  void*                      d_arena = nullptr;
  PuschProcDesc*             d_desc  = nullptr;
  // the workspace, pieces of the arena
  uint32_t*                 d_ce      = nullptr;
  float*                    d_nv      = nullptr;
  nrphy_pusch_chest_meas_t* d_meas    = nullptr;
  float*                    d_sinr    = nullptr;
  int8_t*                   d_llr     = nullptr;
  int8_t*                   d_sch     = nullptr;
  int8_t*                   d_uci_llr = nullptr;
  uint32_t*                 d_dec     = nullptr;
  uint32_t*                 d_status  = nullptr;
  uint8_t*                  d_scratch = nullptr;
  float*                    d_evm     = nullptr; // null unless the plan takes the EVM (nrphy_pusch_evm_plan_create)
};

#pragma GCC visibility push(hidden)

// nrphy_pusch_proc_run in its steps, in its order: the argument check; estimator, demodulator, demultiplexer and UCI decoder;
// the transport-block decoder of plan->decoders[k]; the result kernel.
bool pusch_proc_run_arguments_ok(const nrphy_pusch_proc_plan_t* plan, const void* d_grid, const void* d_harq, const uint8_t* d_tb,
                                 const uint8_t* d_uci_bits, const nrphy_pusch_result_t* d_result);
int pusch_proc_run_front(nrphy_pusch_proc_plan_t* plan, const void* d_grid, uint8_t* d_uci_bits, void* stream);
int pusch_proc_run_decoder(nrphy_pusch_proc_plan_t* plan, size_t k, void* d_harq, uint8_t* d_tb, void* stream);
int pusch_proc_run_result(nrphy_pusch_proc_plan_t* plan, nrphy_pusch_result_t* d_result, void* stream);

#pragma GCC visibility pop
