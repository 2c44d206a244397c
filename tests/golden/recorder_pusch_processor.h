// What record_pusch_processor_reference.cpp and record_pusch_csi2_reference.cpp share: the reference's pusch_processor_impl
// built through its factories, the notifier that keeps its answers, the rx-buffer pool and the 25-PRB grid of a case.
#pragma once

#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "recorder_grid.h"
#include "srsran/phy/generic_functions/generic_functions_factories.h"
#include "srsran/phy/generic_functions/transform_precoding/transform_precoding_factories.h"
#include "srsran/phy/support/time_alignment_estimator/time_alignment_estimator_factories.h"
#include "srsran/phy/upper/channel_coding/channel_coding_factories.h"
#include "srsran/phy/upper/channel_modulation/channel_modulation_factories.h"
#include "srsran/phy/upper/channel_processors/pusch/factories.h"
#include "srsran/phy/upper/channel_processors/pusch/pusch_processor_result_notifier.h"
#include "srsran/phy/upper/channel_processors/uci/factories.h"
#include "srsran/phy/upper/equalization/equalization_factories.h"
#include "srsran/phy/upper/rx_buffer_pool.h"
#include "srsran/phy/upper/sequence_generators/sequence_generator_factories.h"
#include "srsran/phy/upper/signal_processors/signal_processor_factories.h"
#include "srsran/phy/upper/unique_rx_buffer.h"

constexpr unsigned NPRB_GRID = 25, NSUBC = 12 * NPRB_GRID;

// The DFT factory is the recorders' own three lines over dft_processor_generic_impl, because the reference's factory file needs
// FFTW's header.
class dft_factory : public srsran::dft_processor_factory
{
public:
  std::unique_ptr<srsran::dft_processor> create(const srsran::dft_processor::configuration& config) override
  {
    auto dft = std::make_unique<srsran::dft_processor_generic_impl>(config);
    return dft->is_valid() ? std::move(dft) : nullptr;
  }
};

struct Answer : public srsran::pusch_processor_result_notifier {
  bool                                   has_sch = false, has_uci = false;
  srsran::pusch_processor_result_data    sch;
  srsran::pusch_processor_result_control uci;
  void on_uci(const srsran::pusch_processor_result_control& u) override
  {
    uci     = u;
    has_uci = true;
  }
  void on_sch(const srsran::pusch_processor_result_data& s) override
  {
    sch     = s;
    has_sch = true;
  }
};

inline std::unique_ptr<srsran::pusch_processor> make_processor(srsran::channel_equalizer_algorithm_type     eq,
                                                               srsran::channel_state_information::sinr_type sinr)
{
  using namespace srsran;
  auto prg     = create_pseudo_random_generator_sw_factory();
  auto dft     = std::make_shared<dft_factory>();
  auto ta      = create_time_alignment_estimator_dft_factory(dft);
  auto port    = create_port_channel_estimator_factory_sw(ta);
  auto crc     = create_crc_calculator_factory_sw("lut");
  auto dec_cfg = pusch_decoder_factory_sw_configuration{};
  dec_cfg.crc_factory       = crc;
  dec_cfg.decoder_factory   = create_ldpc_decoder_factory_sw("avx2");
  dec_cfg.dematcher_factory = create_ldpc_rate_dematcher_factory_sw("avx2");
  dec_cfg.segmenter_factory = create_ldpc_segmenter_rx_factory_sw();
  dec_cfg.nof_prb           = NPRB_GRID;
  dec_cfg.nof_layers        = 2;
  pusch_processor_factory_sw_configuration cfg;
  cfg.estimator_factory   = create_dmrs_pusch_estimator_factory_sw(prg, port);
  cfg.demodulator_factory = create_pusch_demodulator_factory_sw(create_channel_equalizer_generic_factory(eq),
                                                                create_dft_transform_precoder_factory(dft, NPRB_GRID),
                                                                create_channel_modulation_sw_factory(), prg, NPRB_GRID, false, true);
  cfg.demux_factory       = create_ulsch_demultiplex_factory_sw();
  cfg.decoder_factory     = create_pusch_decoder_factory_sw(dec_cfg);
  cfg.uci_dec_factory     = create_uci_decoder_factory_generic(create_short_block_detector_factory_sw(), create_polar_factory_sw(), crc);
  cfg.ch_estimate_dimensions.nof_prb       = NPRB_GRID;
  cfg.ch_estimate_dimensions.nof_symbols   = 14;
  cfg.ch_estimate_dimensions.nof_rx_ports  = 4;
  cfg.ch_estimate_dimensions.nof_tx_layers = 2;
  cfg.dec_nof_iterations                   = 10;
  cfg.dec_enable_early_stop                = true;
  cfg.max_nof_concurrent_threads           = 1;
  cfg.csi_sinr_calc_method                 = sinr;
  return create_pusch_processor_factory_sw(cfg)->create();
}

inline auto make_rx_buffer_pool()
{
  srsran::rx_buffer_pool_config pool_cfg;
  pool_cfg.max_codeblock_size   = srsran::ldpc::MAX_CODEBLOCK_SIZE;
  pool_cfg.nof_buffers          = 64;
  pool_cfg.nof_codeblocks       = 256;
  pool_cfg.expire_timeout_slots = 1000;
  pool_cfg.external_soft_bits   = false;
  return srsran::create_rx_buffer_pool(pool_cfg);
}

// The case's grid: [ports][14][12 prb_count] words at grid_off of `grids`, from PRB prb_start on; zero outside.
inline word_grid grid_of(const std::vector<uint32_t>& grids, size_t grid_off, unsigned ports, unsigned prb_start, unsigned prb_count)
{
  word_grid grid(ports, NSUBC);
  for (unsigned p = 0; p != ports; ++p) {
    for (unsigned l = 0; l != 14; ++l) {
      for (unsigned k = 0; k != 12 * prb_count; ++k) {
        grid.set(p, l, 12 * prb_start + k, grids[grid_off + (p * 14 + l) * 12 * prb_count + k]);
      }
    }
  }
  return grid;
}
