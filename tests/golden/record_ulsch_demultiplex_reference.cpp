// Records the answers of srsRAN-5G-ER's ulsch_demultiplex_impl for tests/test_ulsch_demultiplex.py.  It constructs the reference's
// class directly, feeds it seeded soft bits with the scrambling sequence of the reference's own generator, and writes the four
// streams it hands to its decoder buffers.  Built and run by oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into
// oracle/_ref/: `make -C oracle recorders`, `make -C oracle rerecord-check`; no binary or object is committed.
//
// Case i is configuration i of the JSON.  Its input is not stored: soft bit k is (mix(seed_i + k) mod 255) - 127 with
// seed_i = 0x9E3779B9 * (i + 1) and mix the 32-bit finaliser of recorder_io.h; rnti = mix(seed_i ^ 0xAAAA) mod 65535 + 1 and
// n_id = mix(seed_i ^ 0x5555) mod 1024.  Files:
//   ulsch_reference_cases.npy  int64 [n][8]: rnti, n_id, soft bits of the codeword, soft bits of the UL-SCH stream, offset of the
//                              case's UCI streams in uci (HARQ-ACK, CSI part 1, CSI part 2 back to back, the configuration's
//                              nof_enc_* each), offset of its UL-SCH stream in sch or -1 where it is not stored, and the
//                              checksum of the UL-SCH stream: the sum of (byte + 129) * (mix(k) | 1) over its bytes, modulo 2^63
//   ulsch_reference_uci.npy    int8, the UCI streams of every case
//   ulsch_reference_sch.npy    int8, the UL-SCH streams of the cases of at most 20000 soft bits
#include "lib/phy/upper/channel_processors/pusch/ulsch_demultiplex_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "recorder_io.h"
#include "srsran/phy/upper/channel_processors/pusch/pusch_decoder_buffer.h"

using namespace srsran;

namespace {

class stream_spy : public pusch_decoder_buffer
{
public:
  std::vector<int8_t> data;
  bool                ended = false;
  span<log_likelihood_ratio> get_next_block_view(unsigned block_size) override
  {
    view.resize(block_size);
    return view;
  }
  void on_new_softbits(span<const log_likelihood_ratio> softbits) override
  {
    for (log_likelihood_ratio v : softbits) {
      data.push_back((int8_t)v.to_int());
    }
  }
  void on_end_softbits() override { ended = true; }

private:
  std::vector<log_likelihood_ratio> view;
};

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s ulsch_demultiplex_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream        json(argv[1]);
  std::string          line;
  std::vector<int64_t> cases;
  std::vector<int8_t>  uci, sch_out;
  unsigned             index = 0;
  while (std::getline(json, line)) {
    if (line.find("\"modulation\"") == std::string::npos) {
      continue;
    }
    ulsch_demultiplex::configuration cfg;
    const unsigned                   code = json_int(line, "modulation");
    cfg.modulation         = code == 0 ? modulation_scheme::PI_2_BPSK : code == 1 ? modulation_scheme::BPSK : code == 2 ? modulation_scheme::QPSK
                             : code == 4 ? modulation_scheme::QAM16 : code == 6 ? modulation_scheme::QAM64 : modulation_scheme::QAM256;
    cfg.nof_layers         = json_int(line, "nof_layers");
    cfg.nof_prb            = json_int(line, "nof_prb");
    cfg.start_symbol_index = json_int(line, "start_symbol_index");
    cfg.nof_symbols        = json_int(line, "nof_symbols");
    cfg.nof_harq_ack_rvd   = json_int(line, "nof_harq_ack_rvd");
    cfg.dmrs               = json_int(line, "dmrs_type") == 0 ? dmrs_type::TYPE1 : dmrs_type::TYPE2;
    const unsigned mask    = json_int(line, "dmrs_symbol_mask");
    cfg.dmrs_symbol_mask   = symbol_slot_mask(14);
    for (unsigned l = 0; l != 14; ++l) {
      cfg.dmrs_symbol_mask.set(l, (mask >> l) & 1U);
    }
    cfg.nof_cdm_groups_without_data = json_int(line, "nof_cdm_groups_without_data");
    cfg.nof_harq_ack_bits           = json_int(line, "nof_harq_ack_bits");
    cfg.nof_enc_harq_ack_bits       = json_int(line, "nof_enc_harq_ack_bits");
    cfg.nof_csi_part1_bits          = json_int(line, "nof_csi_part1_bits");
    cfg.nof_enc_csi_part1_bits      = json_int(line, "nof_enc_csi_part1_bits");
    const unsigned csi2_bits = json_int(line, "nof_csi_part2_bits"), csi2_enc = json_int(line, "nof_enc_csi_part2_bits");

    // The codeword's length: the data REs of every symbol.
    const unsigned nbre    = get_bits_per_symbol(cfg.modulation) * cfg.nof_layers;
    const unsigned re_dmrs = (12 - cfg.nof_cdm_groups_without_data * (cfg.dmrs == dmrs_type::TYPE1 ? 6 : 4)) * cfg.nof_prb;
    unsigned       total   = 0;
    for (unsigned l = cfg.start_symbol_index; l != cfg.start_symbol_index + cfg.nof_symbols; ++l) {
      total += (cfg.dmrs_symbol_mask.test(l) ? re_dmrs : 12 * cfg.nof_prb) * nbre;
    }
    const uint32_t seed = 0x9E3779B9U * (index + 1);
    const unsigned rnti = mix(seed ^ 0xAAAAU) % 65535U + 1, n_id = mix(seed ^ 0x5555U) % 1024U;

    static ulsch_demultiplex_impl demux; // (large: it holds a symbol of soft bits)
    pseudo_random_generator_impl  prg;
    prg.init((rnti << 15) + n_id);
    stream_spy             sch, harq, csi1, csi2;
    pusch_codeword_buffer& cw = demux.demultiplex(sch, harq, csi1, cfg);
    if (csi2_enc != 0) {
      demux.set_csi_part2(csi2, csi2_bits, csi2_enc);
    }
    for (unsigned done = 0; done != total;) {
      span<log_likelihood_ratio> view = cw.get_next_block_view(std::min(total - done, 997U));
      for (unsigned k = 0; k != view.size(); ++k) {
        view[k] = log_likelihood_ratio((int)(mix(seed + done + k) % 255U) - 127);
      }
      dynamic_bit_buffer seq(view.size());
      prg.generate(seq);
      cw.on_new_block(view, seq);
      done += view.size();
    }
    cw.on_end_codeword();
    if (harq.data.size() != cfg.nof_enc_harq_ack_bits || csi1.data.size() != cfg.nof_enc_csi_part1_bits || csi2.data.size() != csi2_enc) {
      std::fprintf(stderr, "case %u: stream sizes\n", index);
      return 1;
    }
    uint64_t sum = 0;
    for (size_t k = 0; k != sch.data.size(); ++k) {
      sum += (uint64_t)(sch.data[k] + 129) * (mix((uint32_t)k) | 1U);
    }
    const bool stored = total <= 20000;
    cases.insert(cases.end(), {(int64_t)rnti, (int64_t)n_id, (int64_t)total, (int64_t)sch.data.size(), (int64_t)uci.size(),
                               stored ? (int64_t)sch_out.size() : -1, (int64_t)(sum & 0x7FFFFFFFFFFFFFFFULL), 0});
    uci.insert(uci.end(), harq.data.begin(), harq.data.end());
    uci.insert(uci.end(), csi1.data.begin(), csi1.data.end());
    uci.insert(uci.end(), csi2.data.begin(), csi2.data.end());
    if (stored) {
      sch_out.insert(sch_out.end(), sch.data.begin(), sch.data.end());
    }
    ++index;
  }
  const std::string out = argv[2];
  write_npy(out + "/ulsch_reference_cases.npy", "<i8", cases, 8);
  write_npy(out + "/ulsch_reference_uci.npy", "|i1", uci, 0);
  write_npy(out + "/ulsch_reference_sch.npy", "|i1", sch_out, 0);
  std::printf("%u cases, %zu UCI soft bits, %zu stored UL-SCH soft bits\n", index, uci.size(), sch_out.size());
  return 0;
}
