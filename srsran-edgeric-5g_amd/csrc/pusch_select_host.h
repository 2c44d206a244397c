// The select-aware forms of the UL-SCH demultiplexer plan (ulsch_host.cpp) and of the UCI decoder plan (uci_host.cpp) behind their
// entry points: what the PUSCH processor with CSI part 2 (pusch_csi2_host.cpp) builds on.  Not part of the ABI.
//
// A plan made here may give each codeword / message a select word and a value.  At run time d_select points to the words; a
// codeword or message whose word does not hold its value does nothing at all -- no stream byte, no payload byte, no status.
// NO_SELECT_WORD (nrphy_internal.h) as the word: unconditional, which is what the entry points make of every codeword and message.
#pragma once

#include "nrphy_host_internal.h"

#pragma GCC visibility push(hidden) // internal to the library

// select_word, select_value: [n], or both null.
int ulsch_demux_plan_create_select(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ulsch_demux_cfg_t* cfgs, const uint64_t* in_offset,
                                   const uint64_t* sch_offset, const uint64_t* harq_offset, const uint64_t* csi1_offset,
                                   const uint64_t* csi2_offset, const uint32_t* select_word, const uint32_t* select_value,
                                   nrphy_ulsch_demux_plan_t** out);
int ulsch_demux_run_select(nrphy_ulsch_demux_plan_t* plan, const int8_t* d_codeword_llr, int8_t* d_sch, int8_t* d_harq_ack,
                           int8_t* d_csi1, int8_t* d_csi2, const uint32_t* d_select, void* stream);

int uci_decoder_plan_create_select(nrphy_ctx_t* ctx, uint32_t n, const nrphy_uci_decoder_cfg_t* cfgs, const uint64_t* llr_offset,
                                   const uint64_t* message_offset, const uint32_t* select_word, const uint32_t* select_value,
                                   nrphy_uci_decoder_plan_t** out);
int uci_decoder_run_select(nrphy_uci_decoder_plan_t* plan, const int8_t* d_llr, uint8_t* d_message, uint32_t* d_status,
                           const uint32_t* d_select, void* stream);

#pragma GCC visibility pop
