// Records the answers of srsRAN-5G-ER's pusch_processor_impl for tests/test_pusch_processor.py.  The processor is built through the
// reference's factories -- create_pusch_processor_factory_sw over the DM-RS estimator (port channel estimator with the time
// alignment estimator on the generic DFT), the demodulator (generic equaliser, ZF or MMSE; no EVM calculator; post-equalisation
// SINR on), the UL-SCH demultiplexer, the UCI decoder (short block detector, polar, CRC) and the software PUSCH decoder (AVX2 LDPC
// decoder and rate dematcher, 10 iterations with early stop) --, reads the received grids the test's transmitter wrote
// (`python tests/test_pusch_processor.py DIR` on a GPU: DIR/inputs_grids.npy, DIR/inputs_cases.txt) and writes one .json and four
// .npy files.  Built and run by oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/, from an archive of
// the reference's library sources: `make -C oracle recorders`, `make -C oracle rerecord-check PUSCH_PROC_INPUTS=DIR`; no binary or
// object is committed.  The recipe says why the build is without fused multiply-adds and why the equaliser alone is compiled
// without AVX2; recorder_pusch_processor.h holds the processor and why its DFT factory is the recorders' own.
//
// Receive ports: as in record_pusch_tp_reference.cpp the reference is handed the list 0 .. n - 1 and a grid whose port i holds what
// receive port i reads.  The grid is 25 PRB wide and zero outside the PDU's allocation, as the test's.
//
// Files (offsets in elements of the named file):
//   pusch_proc_reference_cases.json   per case: pdu (index into "abcdef"), good (1: the SNR at which every block decodes), snr_db,
//                                     equalizer (0 ZF, 1 MMSE), the PDU's fields, prb_start, prb_count, grid_off, tb_off, uci_off
//   pusch_proc_reference_grids.npy    uint32 cbf16 words: per distinct (pdu, good) [rx port][14][12 prb_count]
//   pusch_proc_reference_results.npy  float64 [case][12]: tb_crc_ok, nof_codeblocks_total, harq_ack_status, csi_part1_status
//                                     (uci_status: 0 unknown, 1 valid, 2 invalid), sinr_ch_estimator_dB, sinr_post_eq_dB, epre_dB,
//                                     rsrp_dB, time_alignment_s, has_cfo, cfo_hz, has_sch
//   pusch_proc_reference_tb.npy       uint8: the transport block the decoder delivered (tb_size_bytes per case with a codeword)
//   pusch_proc_reference_uci.npy      uint8: HARQ-ACK then CSI part 1 payload bits, one per byte
#include "recorder_pusch_processor.h"

using namespace srsran;

constexpr unsigned NOF_RESULT = 12;

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
    // the order of write_recorder_inputs() in tests/test_pusch_processor.py
    unsigned pdu_index, good, numerology, slot_index, rnti, n_id, scrambling_id, n_scid, modulation, has_codeword, rv, bg, new_data,
        tb_bytes, lbrm, nharq, ncsi1, start, nsym, dmrs_mask, layers, ports, prb_start, prb_count, equalizer;
    long   dc;
    size_t grid_off;
    double snr_db, rate, alpha, beta_harq, beta_csi1, beta_csi2;
    s >> pdu_index >> good >> snr_db >> numerology >> slot_index >> rnti >> n_id >> scrambling_id >> n_scid >> modulation >> rate >>
        has_codeword >> rv >> bg >> new_data >> tb_bytes >> lbrm >> nharq >> ncsi1 >> alpha >> beta_harq >> beta_csi1 >> beta_csi2 >> start >>
        nsym >> dmrs_mask >> layers >> ports >> dc >> prb_start >> prb_count >> equalizer >> grid_off;

    const word_grid        grid = grid_of(grids, grid_off, ports, prb_start, prb_count);
    pusch_processor::pdu_t pdu;
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

    double row[NOF_RESULT] = {};
    std::vector<uint8_t> tb(tb_bytes, 0);
    for (int pass = 0; pass != 2; ++pass) { // the record keeps one SINR: once per method
      const auto method = pass == 0 ? channel_state_information::sinr_type::channel_estimator
                                    : channel_state_information::sinr_type::post_equalization;
      auto proc = make_processor(equalizer == 0 ? channel_equalizer_algorithm_type::zf : channel_equalizer_algorithm_type::mmse, method);
      unique_rx_buffer buffer;
      if (has_codeword) {
        buffer = pool->get_pool().reserve(pdu.slot, trx_buffer_identifier((uint16_t)(n_case + 1), (uint8_t)pass),
                                          ldpc::compute_nof_codeblocks(units::bytes(tb_bytes).to_bits(), pdu.codeword->ldpc_base_graph), true);
      }
      Answer answer;
      std::fill(tb.begin(), tb.end(), 0);
      proc->process(tb, std::move(buffer), answer, grid, pdu);
      const channel_state_information& csi = has_codeword ? answer.sch.csi : answer.uci.csi;
      if ((has_codeword != 0) != answer.has_sch || ((nharq + ncsi1) != 0) != answer.has_uci) {
        std::fprintf(stderr, "case %u: a result is missing\n", n_case);
        return 1;
      }
      row[4 + pass] = csi.get_sinr_dB().value();
      if (pass == 1) {
        row[0]  = has_codeword && answer.sch.data.tb_crc_ok;
        row[1]  = has_codeword ? answer.sch.data.nof_codeblocks_total : 0;
        row[2]  = nharq ? (double)(int)answer.uci.harq_ack.status : 0;
        row[3]  = ncsi1 ? (double)(int)answer.uci.csi_part1.status : 0;
        row[6]  = csi.get_epre_dB().value();
        row[7]  = csi.get_rsrp_dB().value();
        row[8]  = csi.get_time_alignment().value().to_seconds();
        row[9]  = csi.get_cfo_Hz().has_value();
        row[10] = csi.get_cfo_Hz().value_or(0.0F);
        row[11] = has_codeword;
        for (unsigned b = 0; b != nharq; ++b) {
          ucis.push_back(answer.uci.harq_ack.payload.test(b));
        }
        for (unsigned b = 0; b != ncsi1; ++b) {
          ucis.push_back(answer.uci.csi_part1.payload.test(b));
        }
      }
    }
    json << (n_case ? ",\n" : "") << "{\"pdu\": " << pdu_index << ", \"good\": " << good << ", \"snr_db\": " << snr_db
         << ", \"equalizer\": " << equalizer << ", \"prb_start\": " << prb_start << ", \"prb_count\": " << prb_count
         << ", \"nof_rx_ports\": " << ports << ", \"tb_size_bytes\": " << tb_bytes << ", \"nof_harq_ack\": " << nharq
         << ", \"nof_csi_part1\": " << ncsi1 << ", \"grid_off\": " << grid_off << ", \"tb_off\": " << tbs.size()
         << ", \"uci_off\": " << ucis.size() - nharq - ncsi1 << "}";
    tbs.insert(tbs.end(), tb.begin(), tb.end());
    results.insert(results.end(), row, row + NOF_RESULT);
    ++n_case;
  }
  json << "\n]\n";
  std::ofstream(out + "/pusch_proc_reference_cases.json") << json.str();
  write_npy(out + "/pusch_proc_reference_grids.npy", "<u4", grids, 0);
  write_npy(out + "/pusch_proc_reference_results.npy", "<f8", results, NOF_RESULT);
  write_npy(out + "/pusch_proc_reference_tb.npy", "|u1", tbs, 0);
  write_npy(out + "/pusch_proc_reference_uci.npy", "|u1", ucis, 0);
  std::printf("%u cases\n", n_case);
  return 0;
}
