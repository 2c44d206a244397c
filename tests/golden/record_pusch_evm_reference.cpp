// Records the EVM of srsRAN-5G-ER's pusch_demodulator_impl for tests/test_pusch_evm.py.  It constructs the reference's classes
// directly -- pusch_demodulator_impl with channel_equalizer_generic_impl (ZF or MMSE), demodulation_mapper_impl,
// evm_calculator_generic_impl over modulation_mapper_lut_impl, pseudo_random_generator_impl and transform_precoder_dft_impl over
// the direct-sum dft_processor of record_pusch_tp_reference.cpp --, makes a grid and an estimate per case with that recorder's
// transmitter and channel, and writes inputs and outputs as one .json and eight .npy files.  Its codeword buffer hands back the
// whole request, as every buffer the reference's processor can put behind the demodulator does, so the EVM calculator is
// handed one OFDM symbol's data RE x layers at a time.
//
// Built and run with the committed recipe, whose variables for a recorder may come from the command line (no file under
// oracle/ names this one), against a checkout of srsRAN-5G-ER and into oracle/_ref/; no binary or object is committed:
//
//   make -C oracle recorders RECORDERS=pusch_evm FLAVOUR_pusch_evm=avx2nc \
//     'SRCS_pusch_evm=$(SRCS_pusch_tp) $(U)/channel_modulation/evm_calculator_generic_impl.cpp $(U)/channel_modulation/modulation_mapper_lut_impl.cpp' \
//     'LINK_pusch_evm=$(EQUALIZER_SCALAR)'
//   make -C oracle rerecord-pusch_evm RECORDERS=pusch_evm SELF_CONTAINED=pusch_evm FLAVOUR_pusch_evm=avx2nc \
//     'SRCS_pusch_evm=$(SRCS_pusch_tp) $(U)/channel_modulation/evm_calculator_generic_impl.cpp $(U)/channel_modulation/modulation_mapper_lut_impl.cpp' \
//     'LINK_pusch_evm=$(EQUALIZER_SCALAR)' 'ARGS_pusch_evm=$(RECORDED)'
//   cp oracle/_ref/recorded/pusch_evm_reference_* tests/golden/
//
// The flavour is pusch_tp's for pusch_tp's reasons (oracle/recorders.mk): AVX2 without contraction, the equaliser alone without
// AVX2.  Under it srsvec::dot_prod adds 8 float lanes in sequence, then the lanes in order, then a scalar tail, and a term is
// re * re + im * im with every operation rounded: what tests/pusch_evm_model.py restates.
//
// Cases, in this order (the shapes at which the library's EVM path changes: one and two work items per symbol, DM-RS symbols
// with data, two layers, an RE without estimate, the transform-precoded kernel with one and two rounds of its 256 threads,
// pi/2-BPSK's two tables, and a symbol longer than the calculator's sub-block of 4096):
//   0      1 PRB, 1 layer, 1 port, QPSK, symbols 0-13, DM-RS {2}, 2 CDM groups without data
//   1      22 PRB, 16-QAM, 2 ports, symbols 2-11, DM-RS {2, 11} with 1 CDM group without data (132 data RE on those)
//   2, 3   2 layers on 2 ports with 64-QAM, 2 layers on 4 ports with 256-QAM, PRBs {3, 7, 40}
//   4, 5   an estimate that is zero on one allocated subcarrier, 1 layer and 2 layers
//   6-11   transform precoded, M_rb = 1 and 25, each with pi/2-BPSK, QPSK and 64-QAM (the QPSK one of M_rb = 25 with MMSE)
//   12     pi/2-BPSK without transform precoding
//   13     2 layers x 171 PRB, QPSK, 2 ports: one symbol with data, of 4104 equalised symbols
//
// Files (offsets in elements of the named file; "symbols with data" in ascending order):
//   pusch_evm_reference_cases.json   per case: the configuration as in pusch_tp_reference_cases.json, noise_vars, zero_subc
//                                    (-1: none), grid_off, ce_off, eq_off, z_off (-1: not transform precoded), llr_off, nof_bits,
//                                    sinr_db, and as IEEE-754 bit patterns (exact in JSON) evm_bits, the final stats.evm, and
//                                    provisional_evm_bits, stats.evm of every on_provisional_stats (one per symbol with data)
//   pusch_evm_reference_grids.npy    uint32 cbf16 words: per case [rx port][nof_symbols][12 M_rb], allocated symbols and subcarriers
//   pusch_evm_reference_ce.npy       uint32 cbf16 words: per case [layer][rx port][12 M_rb], the estimate of every allocated symbol
//   pusch_evm_reference_eq.npy       float32 [n][2]: what the equaliser returned, per symbol with data [RE][layer]
//   pusch_evm_reference_z.npy        float32 [n][2]: what the deprecoder returned (transform-precoded cases)
//   pusch_evm_reference_soft.npy     int8: the soft bits as the demapper gave them -- the codeword buffer's block with the
//                                    scrambling sequence on_new_block receives applied again
//   pusch_evm_reference_llr.npy      int8: the codeword buffer's soft bits (descrambled)
//   pusch_evm_reference_tables.npy   float32 [4 + 16 + 64 + 256][2]: modulation_mapper_lut_impl's QPSK, 16-QAM, 64-QAM and
//                                    256-QAM points, entry i of a table = the symbol of the bits of i, first bit highest
#include "lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.h"
#include "lib/phy/upper/channel_modulation/demodulation_mapper_impl.h"
#include "lib/phy/upper/channel_modulation/evm_calculator_generic_impl.h"
#include "lib/phy/upper/channel_modulation/modulation_mapper_lut_impl.h"
#include "lib/phy/upper/channel_processors/pusch/pusch_demodulator_impl.h"
#include "lib/phy/upper/equalization/channel_equalizer_generic_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "recorder_grid.h"
#include "srsran/phy/upper/channel_processors/pusch/pusch_codeword_buffer.h"
#include "srsran/phy/upper/channel_processors/pusch/pusch_demodulator_notifier.h"

#include <cmath>
#include <complex>
#include <random>

using namespace srsran;

namespace {

using cd = std::complex<double>;

uint32_t cbf16_word(cd v)
{
  return bf16_bits((float)v.real()) | (bf16_bits((float)v.imag()) << 16);
}

uint32_t float_bits(float v)
{
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

// The deprecoder's transform: the direct sum in double, rounded once to float.
class dft_direct : public dft_processor
{
  std::vector<cf_t> in, out;
  std::vector<cd>   w;

public:
  explicit dft_direct(unsigned n) : in(n), out(n), w(n)
  {
    for (unsigned k = 0; k != n; ++k) {
      w[k] = std::polar(1.0, 2.0 * M_PI * (double)k / (double)n);
    }
  }
  direction        get_direction() const override { return direction::INVERSE; }
  unsigned         get_size() const override { return (unsigned)in.size(); }
  span<cf_t>       get_input() override { return in; }
  span<const cf_t> run() override
  {
    const size_t n = in.size();
    for (size_t k = 0; k != n; ++k) {
      cd acc = 0.0;
      for (size_t i = 0; i != n; ++i) {
        acc += cd(in[i].real(), in[i].imag()) * w[(i * k) % n];
      }
      out[k] = cf_t((float)acc.real(), (float)acc.imag());
    }
    return out;
  }
};

// Forwarding wrappers that write down what went through them.
struct Log {
  std::vector<float> eq, z;
};
class eq_recorder : public channel_equalizer
{
  std::unique_ptr<channel_equalizer> inner;
  Log&                               log;

public:
  eq_recorder(std::unique_ptr<channel_equalizer> inner_, Log& log_) : inner(std::move(inner_)), log(log_) {}
  void equalize(span<cf_t> eq_symbols, span<float> eq_noise_vars, const re_buffer_reader<cbf16_t>& ch_symbols,
                const ch_est_list& ch_estimates, span<const float> noise_var_estimates, float tx_scaling) override
  {
    inner->equalize(eq_symbols, eq_noise_vars, ch_symbols, ch_estimates, noise_var_estimates, tx_scaling);
    for (cf_t v : eq_symbols) {
      log.eq.push_back(v.real());
      log.eq.push_back(v.imag());
    }
  }
};
class precoder_recorder : public transform_precoder
{
  std::unique_ptr<transform_precoder> inner;
  Log&                                log;

public:
  precoder_recorder(std::unique_ptr<transform_precoder> inner_, Log& log_) : inner(std::move(inner_)), log(log_) {}
  void deprecode_ofdm_symbol(span<cf_t> out, span<const cf_t> in) override
  {
    inner->deprecode_ofdm_symbol(out, in);
    for (cf_t v : out) {
      log.z.push_back(v.real());
      log.z.push_back(v.imag());
    }
  }
};

// A codeword buffer that returns the whole request, and undoes the descrambling of every block it is told about.
class codeword_store : public pusch_codeword_buffer
{
public:
  std::vector<log_likelihood_ratio> data;
  std::vector<int8_t>               soft; // before descrambling
  std::vector<unsigned>             blocks;
  size_t                            used = 0;
  explicit codeword_store(size_t n) : data(n) {}
  span<log_likelihood_ratio> get_next_block_view(unsigned block_size) override
  {
    return span<log_likelihood_ratio>(data).subspan(used, block_size);
  }
  void on_new_block(span<const log_likelihood_ratio> block, const bit_buffer& scrambling_seq) override
  {
    for (unsigned i = 0; i != block.size(); ++i) {
      const int v = block[i].to_int();
      soft.push_back((int8_t)(scrambling_seq.extract(i, 1) ? -v : v));
    }
    blocks.push_back((unsigned)block.size());
    used += block.size();
  }
  void on_end_codeword() override {}
};
class stats_store : public pusch_demodulator_notifier
{
public:
  float              sinr = std::numeric_limits<float>::quiet_NaN(), evm = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> provisional;
  void on_provisional_stats(const demodulation_stats& stats) override { provisional.push_back(stats.evm.value()); }
  void on_end_stats(const demodulation_stats& stats) override
  {
    sinr = stats.sinr_dB.value();
    evm  = stats.evm.value();
  }
};

struct Case {
  int                rnti, n_id, qm, start, nsym;
  std::vector<int>   dmrs;
  int                dmrs_type, cdm, layers;
  std::vector<int>   rx;
  int                equalizer, tp;
  std::vector<int>   prbs;
  std::vector<float> noise; // per receive port
  int                zero;  // 1: the estimate is zero on one allocated subcarrier
};

// rnti, n_id, qm, start, nsym, dmrs symbols, dmrs type, cdm, layers, rx ports, equaliser, tp, prbs, noise per port, zero.
std::vector<Case> all_cases()
{
  return {
      {0x2001, 21, 2, 0, 14, {2}, 1, 2, 1, {0}, 0, 0, {5}, {0.02f}, 0},
      {0x2002, 22, 4, 2, 10, {2, 11}, 1, 1, 1, {0, 1}, 0, 0, range(30, 22), {0.01f, 0.012f}, 0},
      {0x2003, 23, 6, 0, 4, {2}, 1, 2, 2, {0, 1}, 0, 0, {3, 7, 40}, {0.002f, 0.002f}, 0},
      {0x2004, 24, 8, 0, 4, {2}, 1, 2, 2, {0, 1, 2, 3}, 0, 0, {3, 7, 40}, {0.0005f, 0.0004f, 0.0005f, 0.0006f}, 0},
      {0x2005, 25, 2, 3, 3, {4}, 1, 2, 1, {1, 0}, 0, 0, {10, 11}, {0.03f, 0.03f}, 1},
      {0x2006, 26, 4, 3, 3, {4}, 1, 2, 2, {0, 1}, 0, 0, {10, 11}, {0.004f, 0.004f}, 1},
      {0x2007, 27, 1, 0, 4, {1}, 1, 2, 1, {1}, 0, 1, {7}, {0.05f}, 0},
      {0x2008, 28, 2, 0, 4, {1}, 1, 2, 1, {0, 1}, 0, 1, {7}, {0.03f, 0.03f}, 0},
      {0x2009, 29, 6, 0, 4, {1}, 1, 2, 1, {0, 1}, 0, 1, {7}, {0.003f, 0.003f}, 0},
      {0x200A, 30, 1, 1, 4, {2}, 1, 2, 1, {0}, 0, 1, range(20, 25), {0.05f}, 0},
      {0x200B, 31, 2, 1, 4, {2}, 1, 2, 1, {2, 0}, 1, 1, range(20, 25), {0.04f, 0.05f}, 0},
      {0x200C, 32, 6, 1, 4, {2}, 1, 2, 1, {0, 1}, 0, 1, range(20, 25), {0.003f, 0.003f}, 0},
      {0x200D, 33, 1, 4, 3, {5}, 1, 1, 1, {0, 1}, 0, 0, range(12, 3), {0.05f, 0.05f}, 0},
      {0x200E, 34, 2, 0, 2, {0}, 1, 2, 2, {0, 1}, 0, 0, range(0, 171), {0.01f, 0.01f}, 0},
  };
}

// TS 38.211 Section 5.1: one symbol from qm bits.
cd modulate(int qm, const int* b, unsigned i)
{
  auto s = [&](int k) { return 1.0 - 2.0 * b[k]; };
  switch (qm) {
    case 1: {
      const cd x = cd(s(0), s(0)) / std::sqrt(2.0);
      return (i & 1U) ? x * cd(0.0, 1.0) : x;
    }
    case 2:
      return cd(s(0), s(1)) / std::sqrt(2.0);
    case 4:
      return cd(s(0) * (2 - s(2)), s(1) * (2 - s(3))) / std::sqrt(10.0);
    case 6:
      return cd(s(0) * (4 - s(2) * (2 - s(4))), s(1) * (4 - s(3) * (2 - s(5)))) / std::sqrt(42.0);
    default:
      return cd(s(0) * (8 - s(2) * (4 - s(4) * (2 - s(6)))), s(1) * (8 - s(3) * (4 - s(5) * (2 - s(7))))) / std::sqrt(170.0);
  }
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 1;
  }
  const std::string       dir   = argv[1];
  const std::vector<Case> cases = all_cases();

  // The mapper's tables, every index through the mapper itself.
  std::vector<float> tables;
  for (unsigned qm : {2U, 4U, 6U, 8U}) {
    modulation_mapper_lut_impl mapper;
    const unsigned             n = 1U << qm;
    dynamic_bit_buffer         bits(n * qm);
    for (unsigned i = 0; i != n; ++i) {
      bits.insert(i, i * qm, qm);
    }
    std::vector<cf_t> points(n);
    mapper.modulate(points, bits, modulation_scheme(qm));
    for (cf_t v : points) {
      tables.push_back(v.real());
      tables.push_back(v.imag());
    }
  }

  std::vector<uint32_t> grids, ces;
  std::vector<float>    eqs, zs;
  std::vector<int8_t>   llrs, softs;
  std::ofstream         js(dir + "/pusch_evm_reference_cases.json");
  js << "[\n";
  for (size_t ci = 0; ci != cases.size(); ++ci) {
    const Case&    c = cases[ci];
    const unsigned P = (unsigned)c.rx.size(), L = (unsigned)c.layers, M = (unsigned)c.prbs.size(), nsc = 12 * M;
    const unsigned grid_prb = (unsigned)c.prbs.back() + 1, nsubc = 12 * grid_prb;
    std::mt19937   rng(9000 + (unsigned)ci);
    std::normal_distribution<double>       gauss(0.0, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);

    // Channel per (layer, port) on the allocated subcarriers, in order.
    std::vector<unsigned> subc;
    for (int p : c.prbs) {
      for (unsigned k = 0; k != 12; ++k) {
        subc.push_back(12 * (unsigned)p + k);
      }
    }
    std::vector<cd> h(L * P * nsc);
    for (unsigned l = 0; l != L; ++l) {
      for (unsigned p = 0; p != P; ++p) {
        const cd     g0 = std::polar(0.6 + 0.8 * uni(rng), 2.0 * M_PI * uni(rng));
        const cd     g1 = (ci & 1U) ? 0.3 * std::polar(std::abs(g0), 2.0 * M_PI * uni(rng)) : cd(0.0);
        const double d  = 1.0 + std::floor(6.0 * uni(rng));
        for (unsigned j = 0; j != nsc; ++j) {
          h[(l * P + p) * nsc + j] = g0 + g1 * std::polar(1.0, -2.0 * M_PI * d * (double)subc[j] / 4096.0);
        }
      }
    }
    const unsigned zero_j = (unsigned)(uni(rng) * nsc) % nsc; // the zero-channel subcarrier of a case that has one

    word_grid        grid(P, nsubc);
    channel_estimate est({grid_prb, 14, P, L});
    const size_t     grid_off = grids.size(), ce_off = ces.size();
    grids.resize(grid_off + (size_t)P * c.nsym * nsc);
    ces.resize(ce_off + (size_t)L * P * nsc);
    for (unsigned p = 0; p != P; ++p) {
      est.set_noise_variance(c.noise[p], p, 0);
    }
    for (unsigned s = 0; s != (unsigned)c.nsym; ++s) {
      const unsigned sym = (unsigned)c.start + s;
      // Layer symbols on every allocated subcarrier of the symbol (on DM-RS positions nobody reads them).
      std::vector<cd> tx(L * nsc);
      for (unsigned l = 0; l != L; ++l) {
        std::vector<cd> x(nsc);
        for (unsigned j = 0; j != nsc; ++j) {
          int bits[8];
          for (int& b : bits) {
            b = (int)(rng() & 1U);
          }
          x[j] = modulate(c.qm, bits, j);
        }
        if (c.tp) {
          for (unsigned k = 0; k != nsc; ++k) {
            cd acc = 0.0;
            for (unsigned i = 0; i != nsc; ++i) {
              acc += x[i] * std::polar(1.0, -2.0 * M_PI * (double)((size_t)i * k % nsc) / (double)nsc);
            }
            tx[l * nsc + k] = acc / std::sqrt((double)nsc);
          }
        } else {
          std::copy(x.begin(), x.end(), tx.begin() + l * nsc);
        }
      }
      for (unsigned p = 0; p != P; ++p) {
        const double sigma = std::sqrt(std::fabs((double)c.noise[p]) / 2.0);
        for (unsigned j = 0; j != nsc; ++j) {
          cd y = cd(gauss(rng), gauss(rng)) * sigma;
          for (unsigned l = 0; l != L; ++l) {
            y += h[(l * P + p) * nsc + j] * tx[l * nsc + j];
          }
          const uint32_t w                                     = cbf16_word(y);
          grids[grid_off + ((size_t)p * c.nsym + s) * nsc + j] = w;
          grid.set(p, sym, subc[j], w);
          for (unsigned l = 0; l != L; ++l) {
            const uint32_t hw = (c.zero && j == zero_j) ? 0U : cbf16_word(h[(l * P + p) * nsc + j]);
            ces[ce_off + ((size_t)l * P + p) * nsc + j] = hw;
            const cbf16_t hv                            = cbf16_of(hw);
            est.set_ch_estimate(cf_t(to_cf(hv)), subc[j], sym, p, l);
          }
        }
      }
    }

    // The reference, with an EVM calculator.
    Log                                                    log;
    transform_precoder_dft_impl::collection_dft_processors dfts;
    dfts.emplace(M, std::make_unique<dft_direct>(nsc));
    pusch_demodulator_impl demodulator(
        std::make_unique<eq_recorder>(std::make_unique<channel_equalizer_generic_impl>(
                                          c.equalizer ? channel_equalizer_algorithm_type::mmse : channel_equalizer_algorithm_type::zf),
                                      log),
        std::make_unique<precoder_recorder>(std::make_unique<transform_precoder_dft_impl>(std::move(dfts)), log),
        std::make_unique<demodulation_mapper_impl>(),
        std::make_unique<evm_calculator_generic_impl>(std::make_unique<modulation_mapper_lut_impl>()),
        std::make_unique<pseudo_random_generator_impl>(), MAX_RB, true);
    pusch_demodulator::configuration cfg;
    cfg.rnti    = (uint16_t)c.rnti;
    cfg.rb_mask = bounded_bitset<MAX_RB>(grid_prb);
    for (int p : c.prbs) {
      cfg.rb_mask.set((unsigned)p);
    }
    cfg.modulation         = c.qm == 1 ? modulation_scheme::PI_2_BPSK : modulation_scheme(c.qm);
    cfg.start_symbol_index = (unsigned)c.start;
    cfg.nof_symbols        = (unsigned)c.nsym;
    cfg.dmrs_symb_pos      = symbol_slot_mask(14);
    for (int l : c.dmrs) {
      cfg.dmrs_symb_pos.set((unsigned)l);
    }
    cfg.dmrs_config_type            = c.dmrs_type == 1 ? dmrs_type::TYPE1 : dmrs_type::TYPE2;
    cfg.nof_cdm_groups_without_data = (unsigned)c.cdm;
    cfg.n_id                        = (unsigned)c.n_id;
    cfg.nof_tx_layers               = L;
    cfg.enable_transform_precoding  = c.tp != 0;
    for (unsigned p = 0; p != P; ++p) {
      cfg.rx_ports.push_back((uint8_t)p);
    }
    codeword_store cw((size_t)nsc * c.nsym * L * c.qm);
    stats_store    stats;
    demodulator.demodulate(cw, stats, grid, est, cfg);

    const size_t eq_off = eqs.size() / 2, z_off = zs.size() / 2, llr_off = llrs.size();
    eqs.insert(eqs.end(), log.eq.begin(), log.eq.end());
    zs.insert(zs.end(), log.z.begin(), log.z.end());
    for (size_t i = 0; i != cw.used; ++i) {
      llrs.push_back((int8_t)cw.data[i].to_int());
    }
    softs.insert(softs.end(), cw.soft.begin(), cw.soft.end());
    if ((c.tp && log.z.size() != log.eq.size()) || cw.blocks.size() != stats.provisional.size() ||
        log.eq.size() / 2 * (size_t)c.qm != cw.used) {
      std::fprintf(stderr, "case %zu: %zu deprecoded of %zu symbols, %zu blocks, %zu provisional values\n", ci, log.z.size() / 2,
                   log.eq.size() / 2, cw.blocks.size(), stats.provisional.size());
      return 1; // one block per OFDM symbol with data is what the recording is about
    }
    js << "{\"rnti\": " << c.rnti << ", \"n_id\": " << c.n_id << ", \"qm\": " << c.qm << ", \"start_symbol_index\": " << c.start
       << ", \"nof_symbols\": " << c.nsym << ", \"dmrs_symbols\": " << list_json(c.dmrs) << ", \"dmrs_type\": " << c.dmrs_type
       << ", \"nof_cdm_groups_without_data\": " << c.cdm << ", \"nof_tx_layers\": " << c.layers << ", \"rx_ports\": " << list_json(c.rx)
       << ", \"equalizer\": " << c.equalizer << ", \"transform_precoding\": " << c.tp << ", \"prbs\": " << list_json(c.prbs)
       << ", \"noise_vars\": [";
    for (unsigned p = 0; p != P; ++p) {
      char t[32];
      std::snprintf(t, sizeof t, "%s%.9g", p ? ", " : "", (double)c.noise[p]);
      js << t;
    }
    char t[64];
    std::snprintf(t, sizeof t, "%.9g", (double)stats.sinr);
    js << "], \"zero_subc\": " << (c.zero ? (long)subc[zero_j] : -1L) << ", \"grid_off\": " << grid_off << ", \"ce_off\": " << ce_off
       << ", \"eq_off\": " << eq_off << ", \"z_off\": " << (c.tp ? (long)z_off : -1L) << ", \"llr_off\": " << llr_off
       << ", \"nof_bits\": " << cw.used << ", \"sinr_db\": " << (std::isinf(stats.sinr) ? "\"inf\"" : t)
       << ", \"evm_bits\": " << float_bits(stats.evm) << ", \"provisional_evm_bits\": [";
    for (size_t k = 0; k != stats.provisional.size(); ++k) {
      js << (k ? ", " : "") << float_bits(stats.provisional[k]);
    }
    js << "]}" << (ci + 1 == cases.size() ? "\n" : ",\n");
    std::fprintf(stderr, "case %zu: evm %.6f\n", ci, (double)stats.evm);
  }
  js << "]\n";
  write_npy(dir + "/pusch_evm_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pusch_evm_reference_ce.npy", "<u4", ces, 0);
  write_npy(dir + "/pusch_evm_reference_eq.npy", "<f4", eqs, 2);
  write_npy(dir + "/pusch_evm_reference_z.npy", "<f4", zs, 2);
  write_npy(dir + "/pusch_evm_reference_soft.npy", "|i1", softs, 0);
  write_npy(dir + "/pusch_evm_reference_llr.npy", "|i1", llrs, 0);
  write_npy(dir + "/pusch_evm_reference_tables.npy", "<f4", tables, 2);
  std::fprintf(stderr, "%zu cases\n", cases.size());
  return 0;
}
