// Records the answers of srsRAN-5G-ER's pusch_processor_impl for PDUs with a CSI part 2 size description, for
// tests/test_pusch_csi2.py: pdu.uci.csi_part2_size is set, so the processor evaluates uci_part2_get_size on its own decoded CSI
// part 1, redoes get_ulsch_information and tells its demultiplexer and decoder (pusch_processor_impl.cpp:57-86).  The processor is
// built exactly as tests/golden/record_pusch_processor_reference.cpp builds it (ZF, the SINR of the channel estimator;
// recorder_pusch_processor.h), from the same archive of the reference's sources, with the same flags: oracle/recorders.mk,
// `make -C oracle recorders` and `make -C oracle rerecord-check PUSCH_CSI2_INPUTS=DIR`.
//
// DIR holds what `python tests/test_pusch_csi2.py DIR` wrote on a GPU: inputs_grids.npy and inputs_cases.txt, the grids of (g), (h)
// and (i) of tests/pusch_csi2_cases.py for every selectable size at the good SNR and of (h) at -12 dB.  (j) is not recorded: the
// reference's streaming demultiplexer places its part 2 elsewhere than TS 38.212 does.  No binary or object is committed.
// Receive ports and grid as in record_pusch_processor_reference.cpp.
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
#include "recorder_pusch_processor.h"

using namespace srsran;

constexpr unsigned NOF_RESULT = 5;

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s INPUT_DIR OUTPUT_DIR\n", argv[0]);
    return 1;
  }
  const std::string           in = argv[1], out = argv[2];
  const std::vector<uint32_t> grids = read_npy_u32(in + "/inputs_grids.npy");
  std::ifstream               cases(in + "/inputs_cases.txt");
  auto                        pool = make_rx_buffer_pool();

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

    const word_grid grid = grid_of(grids, grid_off, ports, prb_start, prb_count);
    pdu.slot        = slot_point(numerology, slot_index);
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
