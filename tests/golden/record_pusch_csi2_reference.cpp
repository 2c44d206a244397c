// Records the answers of srsRAN-5G-ER's pusch_processor_impl for PDUs with a CSI part 2 size description, for
// tests/test_pusch_csi2.py: pdu.uci.csi_part2_size is set, so the processor evaluates uci_part2_get_size on its own decoded CSI
// part 1, redoes get_ulsch_information and tells its demultiplexer and decoder (pusch_processor_impl.cpp:57-86).  The processor is
// built exactly as tests/golden/record_pusch_processor_reference.cpp builds it (ZF, the SINR of the channel estimator), from the
// same archive of the reference's sources, with the same flags:
//
//   F="-std=c++17 -O2 -ffp-contract=off -DNDEBUG -w -I$R/include -I$R/external/fmt/include -I$R/external -I$R"
//   for every .cpp under $R/lib/{phy/upper,phy/support,phy/generic_functions,srsvec,srslog,ran,support} except *neon*, *fftw*,
//   generic_functions_factories.cpp and what needs further libraries (lib/support/{network,build_info,version,config_yaml}), and
//   $R/external/fmt/src/{format,os}.cc:
//     g++ $F -mavx2 -mfma -c FILE -o OBJ      -- but channel_equalizer_generic_impl.cpp WITHOUT -mavx2 -mfma, and the *avx512*
//     files and crc_calculator_clmul_impl.cpp, which the factories name but this program never selects, with
//     -mavx512f -mavx512bw -mavx512vl -mavx512dq -mavx512vbmi -mpclmul -msse4.1 added
//   ar rcs libref.a OBJ...
//   g++ $F -mavx2 -mfma record_pusch_csi2_reference.cpp libref.a -lpthread -o record_pusch_csi2_reference
//   ./record_pusch_csi2_reference DIR OUT
//
// DIR holds what `python tests/test_pusch_csi2.py DIR` wrote on a GPU: inputs_grids.npy and inputs_cases.txt, the grids of (g), (h)
// and (i) of tests/pusch_csi2_cases.py for every selectable size at the good SNR and of (h) at -12 dB.  (j) is not recorded: the
// reference's streaming demultiplexer places its part 2 elsewhere than TS 38.212 does.  Built and run outside the repository; no
// binary or object is committed.  Receive ports and grid as in record_pusch_processor_reference.cpp.
//
// Files (offsets in elements of the named file):
//   pusch_csi2_reference_cases.json   per case: pdu (index into "ghij"), size (the part 2 bits the transmitter sent), good, snr_db,
//                                     prb_start, prb_count, nof_rx_ports, tb_size_bytes, nof_harq_ack, nof_csi_part1,
//                                     nof_csi_part2 (the bits the REFERENCE reported), grid_off, tb_off, uci_off
//   pusch_csi2_reference_grids.npy    uint32 cbf16 words: per case [rx port][14][12 prb_count]
//   pusch_csi2_reference_results.npy  float64 [case][5]: tb_crc_ok, nof_codeblocks_total, harq_ack_status, csi_part1_status,
//                                     csi_part2_status (uci_status: 0 unknown, 1 valid, 2 invalid)
//   pusch_csi2_reference_tb.npy       uint8: the transport block the decoder delivered
//   pusch_csi2_reference_uci.npy      uint8: HARQ-ACK, CSI part 1, then CSI part 2 payload bits, one per byte
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "srsran/phy/generic_functions/generic_functions_factories.h"
#include "srsran/phy/generic_functions/transform_precoding/transform_precoding_factories.h"
#include "srsran/phy/support/resource_grid_reader.h"
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

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace srsran;

namespace {

constexpr unsigned NPRB_GRID = 25, NSUBC = 12 * NPRB_GRID, NOF_RESULT = 5;

template <typename T>
void write_npy(const std::string& path, const char* descr, const std::vector<T>& data, size_t cols)
{
  std::ostringstream shape;
  if (cols == 0) {
    shape << "(" << data.size() << ",)";
  } else {
    shape << "(" << data.size() / cols << ", " << cols << ")";
  }
  std::string header = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape.str() + ", }";
  while ((10 + header.size() + 1) % 64 != 0) {
    header += ' ';
  }
  header += '\n';
  std::ofstream  f(path, std::ios::binary);
  const char     magic[8] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0};
  const uint16_t len      = (uint16_t)header.size();
  f.write(magic, 8);
  f.write((const char*)&len, 2);
  f.write(header.data(), header.size());
  f.write((const char*)data.data(), data.size() * sizeof(T));
}

std::vector<uint32_t> read_npy_u32(const std::string& path)
{
  std::ifstream f(path, std::ios::binary);
  char          head[10];
  f.read(head, 10);
  const unsigned len = (unsigned char)head[8] | ((unsigned char)head[9] << 8);
  f.seekg(10 + len);
  std::vector<char>     bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<uint32_t> out(bytes.size() / 4);
  std::memcpy(out.data(), bytes.data(), out.size() * 4);
  return out;
}

cbf16_t cbf16_of(uint32_t w)
{
  uint32_t lo = w << 16, hi = w & 0xFFFF0000U;
  float    re, im;
  std::memcpy(&re, &lo, 4);
  std::memcpy(&im, &hi, 4);
  return cbf16_t(re, im); // exact: the halves are bf16 values
}

// A grid [ports][14][NSUBC] of cbf16 behind the reference's reader interface.
class word_grid : public resource_grid_reader
{
public:
  unsigned             ports;
  std::vector<cbf16_t> re;

  explicit word_grid(unsigned ports_) : ports(ports_), re(ports_ * 14 * NSUBC) {}
  cbf16_t&   at(unsigned port, unsigned l, unsigned k) { return re[(port * 14 + l) * NSUBC + k]; }
  unsigned   get_nof_ports() const override { return ports; }
  unsigned   get_nof_subc() const override { return NSUBC; }
  unsigned   get_nof_symbols() const override { return 14; }
  bool       is_empty(unsigned) const override { return false; }
  bool       is_empty() const override { return false; }
  span<cf_t> get(span<cf_t> symbols, unsigned port, unsigned l, unsigned k_init, const bounded_bitset<MAX_RB * NRE>& mask) const override
  {
    unsigned n = 0;
    mask.for_each(0, mask.size(), [&](unsigned k) { symbols[n++] = to_cf(re[(port * 14 + l) * NSUBC + k_init + k]); });
    return symbols.last(symbols.size() - n);
  }
  span<cbf16_t> get(span<cbf16_t> symbols, unsigned port, unsigned l, unsigned k_init, const bounded_bitset<MAX_RB * NRE>& mask) const override
  {
    unsigned n = 0;
    mask.for_each(0, mask.size(), [&](unsigned k) { symbols[n++] = re[(port * 14 + l) * NSUBC + k_init + k]; });
    return symbols.last(symbols.size() - n);
  }
  void get(span<cf_t> symbols, unsigned port, unsigned l, unsigned k_init, unsigned stride) const override
  {
    for (unsigned k = 0; k != symbols.size(); ++k) {
      symbols[k] = to_cf(re[(port * 14 + l) * NSUBC + k_init + k * stride]);
    }
  }
  void get(span<cbf16_t> symbols, unsigned port, unsigned l, unsigned k_init) const override
  {
    for (unsigned k = 0; k != symbols.size(); ++k) {
      symbols[k] = re[(port * 14 + l) * NSUBC + k_init + k];
    }
  }
  span<const cbf16_t> get_view(unsigned port, unsigned l) const override
  {
    return span<const cbf16_t>(re).subspan((port * 14 + l) * NSUBC, NSUBC);
  }
};

class dft_factory : public dft_processor_factory
{
public:
  std::unique_ptr<dft_processor> create(const dft_processor::configuration& config) override
  {
    auto dft = std::make_unique<dft_processor_generic_impl>(config);
    return dft->is_valid() ? std::move(dft) : nullptr;
  }
};

struct Answer : public pusch_processor_result_notifier {
  bool                           has_sch = false, has_uci = false;
  pusch_processor_result_data    sch;
  pusch_processor_result_control uci;
  void on_uci(const pusch_processor_result_control& u) override
  {
    uci     = u;
    has_uci = true;
  }
  void on_sch(const pusch_processor_result_data& s) override
  {
    sch     = s;
    has_sch = true;
  }
};

std::unique_ptr<pusch_processor> make_processor(channel_equalizer_algorithm_type eq, channel_state_information::sinr_type sinr)
{
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

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s INPUT_DIR OUTPUT_DIR\n", argv[0]);
    return 1;
  }
  const std::string           in = argv[1], out = argv[2];
  const std::vector<uint32_t> grids = read_npy_u32(in + "/inputs_grids.npy");
  std::ifstream               cases(in + "/inputs_cases.txt");
  rx_buffer_pool_config       pool_cfg;
  pool_cfg.max_codeblock_size   = ldpc::MAX_CODEBLOCK_SIZE;
  pool_cfg.nof_buffers          = 64;
  pool_cfg.nof_codeblocks       = 256;
  pool_cfg.expire_timeout_slots = 1000;
  pool_cfg.external_soft_bits   = false;
  auto pool = create_rx_buffer_pool(pool_cfg);

  std::vector<double>  results;
  std::vector<uint8_t> tbs, ucis;
  std::ostringstream   json;
  json << "[\n";
  std::string line;
  unsigned    n_case = 0;
  while (std::getline(cases, line)) {
    if (line.empty()) {
      continue;
    }
    std::istringstream s(line);
    // the order of write_recorder_inputs() in tests/test_pusch_csi2.py
    unsigned pdu_index, size, good, numerology, slot_index, rnti, n_id, scrambling_id, n_scid, modulation, has_codeword, rv, bg, new_data,
        tb_bytes, lbrm, nharq, ncsi1, start, nsym, dmrs_mask, layers, ports, prb_start, prb_count, nof_entries;
    long   dc;
    size_t grid_off;
    double snr_db, rate, alpha, beta_harq, beta_csi1, beta_csi2;
    s >> pdu_index >> size >> good >> snr_db >> numerology >> slot_index >> rnti >> n_id >> scrambling_id >> n_scid >> modulation >> rate >>
        has_codeword >> rv >> bg >> new_data >> tb_bytes >> lbrm >> nharq >> ncsi1 >> alpha >> beta_harq >> beta_csi1 >> beta_csi2 >> start >>
        nsym >> dmrs_mask >> layers >> ports >> dc >> prb_start >> prb_count >> grid_off >> nof_entries;

    pusch_processor::pdu_t pdu;
    for (unsigned e = 0; e != nof_entries; ++e) { // nof_parameters, then (offset, width) each, map_size, then the map
      uci_part2_size_description::entry& entry = pdu.uci.csi_part2_size.entries.emplace_back();
      unsigned nof_parameters, map_size;
      s >> nof_parameters;
      for (unsigned k = 0; k != nof_parameters; ++k) {
        unsigned offset, width;
        s >> offset >> width;
        entry.parameters.push_back({(uint16_t)offset, (uint8_t)width});
      }
      s >> map_size;
      for (unsigned k = 0; k != map_size; ++k) {
        unsigned v;
        s >> v;
        entry.map.push_back((uint16_t)v);
      }
    }
    if (!s) {
      std::fprintf(stderr, "case %u: a short line\n", n_case);
      return 1;
    }

    word_grid grid(ports);
    for (unsigned p = 0; p != ports; ++p) {
      for (unsigned l = 0; l != 14; ++l) {
        for (unsigned k = 0; k != 12 * prb_count; ++k) {
          grid.at(p, l, 12 * prb_start + k) = cbf16_of(grids[grid_off + (p * 14 + l) * 12 * prb_count + k]);
        }
      }
    }
    pdu.slot         = slot_point(numerology, slot_index);
    pdu.rnti         = rnti;
    pdu.bwp_size_rb  = NPRB_GRID;
    pdu.bwp_start_rb = 0;
    pdu.cp           = cyclic_prefix::NORMAL;
    pdu.mcs_descr    = {modulation == 2 ? modulation_scheme::QPSK : modulation == 4 ? modulation_scheme::QAM16 : modulation_scheme::QAM64,
                        (float)rate};
    if (has_codeword) {
      pdu.codeword = pusch_processor::codeword_description{rv, bg == 1 ? ldpc_base_graph_type::BG1 : ldpc_base_graph_type::BG2, new_data != 0};
    }
    pdu.uci.nof_harq_ack          = nharq;
    pdu.uci.nof_csi_part1         = ncsi1;
    pdu.uci.alpha_scaling         = (float)alpha;
    pdu.uci.beta_offset_harq_ack  = (float)beta_harq;
    pdu.uci.beta_offset_csi_part1 = (float)beta_csi1;
    pdu.uci.beta_offset_csi_part2 = (float)beta_csi2;
    pdu.n_id                      = n_id;
    pdu.nof_tx_layers             = layers;
    for (unsigned p = 0; p != ports; ++p) {
      pdu.rx_ports.push_back(p);
    }
    pdu.dmrs_symbol_mask = symbol_slot_mask(14);
    for (unsigned l = 0; l != 14; ++l) {
      if ((dmrs_mask >> l) & 1U) {
        pdu.dmrs_symbol_mask.set(l);
      }
    }
    pdu.dmrs                        = dmrs_type::TYPE1;
    pdu.scrambling_id               = scrambling_id;
    pdu.n_scid                      = n_scid != 0;
    pdu.nof_cdm_groups_without_data = 2;
    pdu.freq_alloc                  = rb_allocation::make_type1(prb_start, prb_count);
    pdu.start_symbol_index          = start;
    pdu.nof_symbols                 = nsym;
    pdu.tbs_lbrm                    = units::bytes(lbrm);
    if (dc >= 0) {
      pdu.dc_position = (unsigned)dc;
    }

    std::vector<uint8_t> tb(tb_bytes, 0);
    auto proc = make_processor(channel_equalizer_algorithm_type::zf, channel_state_information::sinr_type::channel_estimator);
    unique_rx_buffer buffer = pool->get_pool().reserve(pdu.slot, trx_buffer_identifier((uint16_t)(n_case + 1), 0),
                                                       ldpc::compute_nof_codeblocks(units::bytes(tb_bytes).to_bits(), pdu.codeword->ldpc_base_graph), true);
    Answer answer;
    proc->process(tb, std::move(buffer), answer, grid, pdu);
    if (!answer.has_sch || !answer.has_uci) {
      std::fprintf(stderr, "case %u: a result is missing\n", n_case);
      return 1;
    }
    const unsigned ncsi2 = (unsigned)answer.uci.csi_part2.payload.size();
    const double   row[NOF_RESULT] = {(double)answer.sch.data.tb_crc_ok, (double)answer.sch.data.nof_codeblocks_total,
                                      nharq ? (double)(int)answer.uci.harq_ack.status : 0, (double)(int)answer.uci.csi_part1.status,
                                      (double)(int)answer.uci.csi_part2.status};
    const size_t uci_off = ucis.size();
    for (unsigned b = 0; b != nharq; ++b) {
      ucis.push_back(answer.uci.harq_ack.payload.test(b));
    }
    for (unsigned b = 0; b != ncsi1; ++b) {
      ucis.push_back(answer.uci.csi_part1.payload.test(b));
    }
    for (unsigned b = 0; b != ncsi2; ++b) {
      ucis.push_back(answer.uci.csi_part2.payload.test(b));
    }
    json << (n_case ? ",\n" : "") << "{\"pdu\": " << pdu_index << ", \"size\": " << size << ", \"good\": " << good << ", \"snr_db\": " << snr_db
         << ", \"prb_start\": " << prb_start << ", \"prb_count\": " << prb_count << ", \"nof_rx_ports\": " << ports
         << ", \"tb_size_bytes\": " << tb_bytes << ", \"nof_harq_ack\": " << nharq << ", \"nof_csi_part1\": " << ncsi1
         << ", \"nof_csi_part2\": " << ncsi2 << ", \"grid_off\": " << grid_off << ", \"tb_off\": " << tbs.size() << ", \"uci_off\": " << uci_off
         << "}";
    tbs.insert(tbs.end(), tb.begin(), tb.end());
    results.insert(results.end(), row, row + NOF_RESULT);
    ++n_case;
  }
  json << "\n]\n";
  std::ofstream(out + "/pusch_csi2_reference_cases.json") << json.str();
  write_npy(out + "/pusch_csi2_reference_grids.npy", "<u4", grids, 0);
  write_npy(out + "/pusch_csi2_reference_results.npy", "<f8", results, NOF_RESULT);
  write_npy(out + "/pusch_csi2_reference_tb.npy", "|u1", tbs, 0);
  write_npy(out + "/pusch_csi2_reference_uci.npy", "|u1", ucis, 0);
  std::printf("%u cases\n", n_case);
  return 0;
}
