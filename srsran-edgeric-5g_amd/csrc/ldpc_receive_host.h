// The batch forms of the rate dematcher (ldpc_dematcher_host.cpp) and of the LDPC decoder (ldpc_decoder_host.cpp) behind
// their entry points: what the PUSCH transport-block decoder (pusch_decoder_host.cpp) builds on.  Not part of the ABI.
#pragma once

#include "nrphy_host_internal.h"

#include <vector>

#pragma GCC visibility push(hidden) // internal to the library

// The walk of ldpc_rate_dematcher_impl::allot_llrs (ldpc_rate_dematcher_impl.cpp:118-200) over the soft buffer, with
// the data taken out: which ranges it clears, fills, copies into and adds to, in its order.
void build_dematch_ops(std::vector<DematchOp>& ops, unsigned block_length, unsigned buffer_length, unsigned k0,
                       unsigned nof_systematic, unsigned nof_filler, unsigned e, bool new_data);

// n_outer groups (transport blocks) of n_cb codeblocks: codeblock (g, i) reads d_in + g * in_outer + i * in_stride and
// owns the soft buffer d_soft + g * soft_outer + i * soft_stride.  d_select (may be null: unconditional): the launch acts only
// when the word it points to holds select_value at the time the kernel runs.
int rate_dematch_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb, uint32_t n_outer,
                       const int8_t* d_in, uint32_t in_stride_bytes, size_t in_outer, int8_t* d_soft,
                       uint32_t soft_stride_bytes, size_t soft_outer, int new_data, void* stream,
                       const uint32_t* d_select = nullptr, uint32_t select_value = 0);

// skip / ok_flags: per-codeblock HARQ state of a transport-block decoder; crc_at_end: no early stop.
// expected_extent: how many of the nof_llr soft bits the caller expects to be in use (the rest zero), 0 = all of them; it
// only sizes the launch's LDS (messages per edge in LDS when the layers that extent needs are few), never the result.
int ldpc_decode_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb, const int8_t* d_llr,
                      uint32_t llr_stride_bytes, uint8_t* d_out, uint32_t out_stride_bytes, uint32_t* d_iterations,
                      const uint8_t* d_skip, uint8_t* d_ok_flags, bool crc_at_end, void* d_scratch, void* stream,
                      uint32_t expected_extent = 0);

// The HARQ block sizes and the codeblock count nrphy_pusch_decoder_sizes gives, without a context (pusch_decoder_host.cpp):
// false for a configuration the decoder refuses.  No device work.
bool pusch_decoder_harq_sizes(const nrphy_pusch_decoder_cfg_t& cfg, uint32_t n_tb, uint64_t* soft_bytes_per_tb, uint64_t* state_bytes,
                              uint32_t* nof_codeblocks);

// nrphy_pusch_decode_batch for one transport block whose rate-matched length is one of nof_variants candidates, chosen on the
// device: variant v is the configuration cfgs[v] (all equal but for nof_ch_symbols) reading its soft bits at d_llr[v], and its
// rate-dematcher launches act only when *d_select == select_values[v]; the LDPC decode and the assembly, which do not depend on
// the rate-matched length, are launched once.  d_select null with one variant: nrphy_pusch_decode_batch itself.
struct PuschDecodeVariant {
  const nrphy_pusch_decoder_cfg_t* cfg;
  const int8_t*                    d_llr;
  uint32_t                         select_value;
};
int pusch_decode_variants(nrphy_ctx_t* ctx, const PuschDecodeVariant* variants, uint32_t nof_variants, const uint32_t* d_select,
                          uint32_t n_tb, uint64_t llr_stride_bytes, int8_t* d_soft, uint8_t* d_state, void* d_scratch, uint8_t* d_tb,
                          uint32_t tb_stride_bytes, uint32_t* d_result, void* stream);

#pragma GCC visibility pop
