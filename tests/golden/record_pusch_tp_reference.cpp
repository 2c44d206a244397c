// Records the answers of srsRAN-5G-ER's pusch_demodulator_impl with transform precoding and with pi/2-BPSK for
// tests/test_pusch_transform_precoding.py.  It constructs the reference's classes directly -- pusch_demodulator_impl with
// channel_equalizer_generic_impl (ZF or MMSE), demodulation_mapper_impl, pseudo_random_generator_impl, no EVM calculator, and
// transform_precoder_dft_impl over a dft_processor of this program's own: the direct sum in double, rounded once to float (the
// reference's deprecoder needs a dft_processor for sizes its generic implementation does not have; its unit test uses FFTW) --,
// makes a grid and an estimate per case with a transmitter and channel of its own, and writes inputs and outputs as one .json and
// six .npy files.  Built and run by oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/:
// `make -C oracle recorders`, `make -C oracle rerecord-check`; no binary or object is committed.  The recipe says why the build
// is without fused multiply-adds and why the equaliser alone is compiled without AVX2.
//
// Receive ports.  pusch_demodulator_impl reads a contiguous allocation through grid.get_view(i_port, ...) -- the port's position
// in the list -- and any other through grid.get(..., rx_ports[i_port], ...) -- its identifier (pusch_demodulator_impl.h:104-128).
// A case is recorded as what the list means, receive port i reads grid port rx_ports[i]: the reference is handed the list
// 0 .. n - 1 and a grid whose port i holds that data.
//
// Cases, in this order:
//   group 0  the 14 transform-precoded and the 6 plain pi/2-BPSK configurations of pusch_demodulator_configs.json, each with ZF and
//            -- one layer only, as the reference's equaliser -- with MMSE
//   group 1  the small shapes of small_shapes() below: M_rb = 1, 5, 25, 27, 270 and a non-contiguous 6, every modulation, 1 to 4
//            ports, rx_ports = (2, 0), a port with an invalid noise variance, and two plain PUSCHs
//
// The transmitter: random bits mapped to the case's constellation (TS 38.211 Section 5.1), per data OFDM symbol of a
// transform-precoded case the precoding of Section 6.3.1.4 in double, y(k) = sum_i x(i) exp(-j 2 pi i k / M_sc) / sqrt(M_sc).  The
// channel: per (layer, receive port) a gain of amplitude 0.6 .. 1.4 and any phase, on odd-numbered cases a second tap of 0.3 times
// that, 1 to 6 samples of a 4096-point transform later; complex Gaussian noise of the case's noise variance per port (the
// configuration's noise_var); every grid and estimate element rounded to bf16 (nearest, ties to even).  The estimate is the
// channel, zero on one allocated subcarrier per case (its RE are the symbol 0 with variance +inf).
//
// Files (all offsets in elements of the named file; "symbols with data" in ascending order):
//   pusch_tp_reference_cases.json   per case: group, the configuration (rnti, n_id, qm, start_symbol_index, nof_symbols,
//                                   dmrs_symbols, dmrs_type, nof_cdm_groups_without_data, nof_tx_layers, rx_ports, equalizer (0 ZF,
//                                   1 MMSE), transform_precoding, prbs), noise_vars per receive port, grid_off, ce_off, eq_off,
//                                   z_off (-1: not transform precoded), llr_off, nof_bits, sinr_db
//   pusch_tp_reference_grids.npy    uint32 cbf16 words (re in the low half): per case [rx port][nof_symbols][12 M_rb], the
//                                   allocated symbols and the subcarriers of the allocated PRBs in ascending order
//   pusch_tp_reference_ce.npy       uint32 cbf16 words: per case [layer][rx port][12 M_rb], the estimate of every allocated symbol
//   pusch_tp_reference_eq.npy       float32 [n][2]: what the equaliser returned, per symbol with data [RE][layer]
//   pusch_tp_reference_nvar.npy     float32: its noise variances, in the same order
//   pusch_tp_reference_z.npy        float32 [n][2]: what the deprecoder returned, per symbol with data (transform-precoded cases)
//   pusch_tp_reference_llr.npy      int8: the codeword buffer's soft bits
#include "lib/phy/generic_functions/transform_precoding/transform_precoder_dft_impl.h"
#include "lib/phy/upper/channel_modulation/demodulation_mapper_impl.h"
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
  std::vector<float> eq, nvar, z;
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
    log.nvar.insert(log.nvar.end(), eq_noise_vars.begin(), eq_noise_vars.end());
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
    inner->deprecode_ofdm_symbol(out, in); // its input is the equaliser's output, written down there
    for (cf_t v : out) {
      log.z.push_back(v.real());
      log.z.push_back(v.imag());
    }
  }
};

// A codeword buffer that hands out whole-symbol views, as the reference's test double does.
class codeword_store : public pusch_codeword_buffer
{
public:
  std::vector<log_likelihood_ratio> data;
  size_t                            used = 0;
  explicit codeword_store(size_t n) : data(n) {}
  span<log_likelihood_ratio> get_next_block_view(unsigned block_size) override
  {
    return span<log_likelihood_ratio>(data).subspan(used, block_size);
  }
  void on_new_block(span<const log_likelihood_ratio> block, const bit_buffer&) override { used += block.size(); }
  void on_end_codeword() override {}
};
class stats_store : public pusch_demodulator_notifier
{
public:
  float sinr = std::numeric_limits<float>::quiet_NaN();
  void  on_provisional_stats(const demodulation_stats&) override {}
  void  on_end_stats(const demodulation_stats& stats) override { sinr = stats.sinr_dB.value(); }
};

struct Case {
  int              group, rnti, n_id, qm, start, nsym;
  std::vector<int> dmrs;
  int              dmrs_type, cdm, layers;
  std::vector<int> rx;
  int              equalizer, tp;
  std::vector<int> prbs;
  std::vector<float> noise; // per receive port
};

// group, rnti, n_id, qm, start, nsym, dmrs symbols, dmrs type, cdm, layers, rx ports, equaliser, tp, prbs, noise per port.
std::vector<Case> small_shapes()
{
  return {
      {1, 0x1001, 11, 1, 0, 4, {1}, 1, 2, 1, {1}, 0, 1, {7}, {0.02f}},                                       // one stage pair, pi/2-BPSK
      {1, 0x1002, 12, 8, 2, 4, {3}, 1, 2, 1, {2, 0}, 1, 1, range(10, 5), {0.002f, 0.003f}},                  // the first factor 5
      {1, 0x1003, 13, 2, 1, 4, {2}, 1, 2, 1, {0, 1, 3}, 0, 1, range(20, 25), {0.05f, -1.0f, 0.04f}},         // 5^2; port 1 invalid
      {1, 0x1004, 14, 6, 0, 4, {0}, 1, 2, 1, {3, 1, 0, 2}, 1, 1, range(50, 27), {0.01f, 0.012f, 0.008f, 0.01f}}, // 3^4, four ports
      {1, 0x1005, 15, 8, 2, 2, {2}, 1, 2, 1, {0}, 0, 1, range(0, 270), {0.001f}},                            // the largest size
      {1, 0x1006, 16, 4, 5, 3, {6}, 1, 2, 1, {2, 0}, 0, 1, {3, 4, 9, 100, 101, 200}, {0.01f, 0.02f}},        // non-contiguous
      {1, 0x1007, 17, 1, 3, 3, {4}, 1, 2, 1, {2, 0}, 1, 1, range(60, 5), {0.03f, 0.02f}},                    // pi/2-BPSK, MMSE
      {1, 0x1008, 18, 6, 0, 4, {2}, 1, 1, 2, {0, 1}, 0, 0, range(30, 23), {0.004f, 0.004f}},                 // plain, two chunks
      {1, 0x1009, 19, 2, 4, 3, {5}, 2, 1, 1, {1, 2, 3}, 1, 0, range(100, 22), {0.05f, 0.06f, 0.05f}},        // plain
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
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s pusch_demodulator_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream     in(argv[1]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  const std::string text = buffer.str();
  const std::string dir  = argv[2];

  std::vector<Case> cases;
  const std::regex  object("\\{\"noise_var\"[^}]*\\}"); // up to the end of "estimate_dims"
  for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it) {
    const std::string o  = it->str();
    const bool        tp = o.find("\"transform_precoding\": true") != std::string::npos;
    std::smatch       m;
    std::regex_search(o, m, std::regex("\"modulation\": \"([A-Z0-9_]+)\""));
    const std::string mod = m[1];
    const int         qm  = mod == "PI_2_BPSK" ? 1 : mod == "QPSK" ? 2 : mod == "QAM16" ? 4 : mod == "QAM64" ? 6 : 8;
    if (!tp && qm != 1) {
      continue;
    }
    std::regex_search(o, m, std::regex("\"noise_var\": ([0-9.eE+-]+)"));
    const float nv = std::stof(m[1]);
    Case        c  = {0, json_int(o, "rnti"), json_int(o, "n_id"), qm, json_int(o, "start_symbol_index"), json_int(o, "nof_symbols"),
                      json_list(o, "dmrs_symbols"), json_int(o, "dmrs_type"), json_int(o, "nof_cdm_groups_without_data"),
                      json_int(o, "nof_tx_layers"), json_list(o, "rx_ports"), 0, tp ? 1 : 0, json_list(o, "rb_mask"), {}};
    c.noise.assign(c.rx.size(), nv);
    for (int eq = 0; eq != (c.layers == 1 ? 2 : 1); ++eq) {
      c.equalizer = eq;
      cases.push_back(c);
    }
  }
  std::fprintf(stderr, "%zu cases of the reference's configurations\n", cases.size());
  for (const Case& c : small_shapes()) {
    cases.push_back(c);
  }

  std::vector<uint32_t> grids, ces;
  std::vector<float>    eqs, nvars, zs;
  std::vector<int8_t>   llrs;
  std::ofstream         js(dir + "/pusch_tp_reference_cases.json");
  js << "[\n";
  for (size_t ci = 0; ci != cases.size(); ++ci) {
    const Case&    c = cases[ci];
    const unsigned P = (unsigned)c.rx.size(), L = (unsigned)c.layers, M = (unsigned)c.prbs.size(), nsc = 12 * M;
    const unsigned grid_prb = (unsigned)c.prbs.back() + 1, nsubc = 12 * grid_prb;
    std::mt19937   rng(7000 + (unsigned)ci);
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
    const unsigned zero_j = (unsigned)(uni(rng) * nsc) % nsc; // the zero-channel subcarrier

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
          const uint32_t w                                       = cbf16_word(y);
          grids[grid_off + ((size_t)p * c.nsym + s) * nsc + j] = w;
          grid.set(p, sym, subc[j], w);
          for (unsigned l = 0; l != L; ++l) {
            const uint32_t hw = j == zero_j ? 0U : cbf16_word(h[(l * P + p) * nsc + j]);
            ces[ce_off + ((size_t)l * P + p) * nsc + j]                = hw;
            const cbf16_t hv                                         = cbf16_of(hw);
            est.set_ch_estimate(cf_t(to_cf(hv)), subc[j], sym, p, l);
          }
        }
      }
    }

    // The reference.
    Log                                                  log;
    transform_precoder_dft_impl::collection_dft_processors dfts;
    dfts.emplace(M, std::make_unique<dft_direct>(nsc));
    pusch_demodulator_impl demodulator(
        std::make_unique<eq_recorder>(std::make_unique<channel_equalizer_generic_impl>(
                                          c.equalizer ? channel_equalizer_algorithm_type::mmse : channel_equalizer_algorithm_type::zf),
                                      log),
        std::make_unique<precoder_recorder>(std::make_unique<transform_precoder_dft_impl>(std::move(dfts)), log),
        std::make_unique<demodulation_mapper_impl>(), nullptr, std::make_unique<pseudo_random_generator_impl>(), MAX_RB, true);
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

    const size_t eq_off = nvars.size(), z_off = zs.size() / 2, llr_off = llrs.size();
    eqs.insert(eqs.end(), log.eq.begin(), log.eq.end());
    nvars.insert(nvars.end(), log.nvar.begin(), log.nvar.end());
    zs.insert(zs.end(), log.z.begin(), log.z.end());
    for (size_t i = 0; i != cw.used; ++i) {
      llrs.push_back((int8_t)cw.data[i].to_int());
    }
    if (c.tp && log.z.size() != log.eq.size()) {
      std::fprintf(stderr, "case %zu: the deprecoder saw %zu of %zu symbols\n", ci, log.z.size() / 2, log.eq.size() / 2);
      return 1;
    }
    js << "{\"group\": " << c.group << ", \"rnti\": " << c.rnti << ", \"n_id\": " << c.n_id << ", \"qm\": " << c.qm
       << ", \"start_symbol_index\": " << c.start << ", \"nof_symbols\": " << c.nsym << ", \"dmrs_symbols\": " << list_json(c.dmrs)
       << ", \"dmrs_type\": " << c.dmrs_type << ", \"nof_cdm_groups_without_data\": " << c.cdm << ", \"nof_tx_layers\": " << c.layers
       << ", \"rx_ports\": " << list_json(c.rx) << ", \"equalizer\": " << c.equalizer << ", \"transform_precoding\": " << c.tp
       << ", \"prbs\": " << list_json(c.prbs) << ", \"noise_vars\": [";
    for (unsigned p = 0; p != P; ++p) {
      char t[32];
      std::snprintf(t, sizeof t, "%s%.9g", p ? ", " : "", (double)c.noise[p]);
      js << t;
    }
    char t[64];
    std::snprintf(t, sizeof t, "%.9g", (double)stats.sinr);
    js << "], \"grid_off\": " << grid_off << ", \"ce_off\": " << ce_off << ", \"eq_off\": " << eq_off
       << ", \"z_off\": " << (c.tp ? (long)z_off : -1L) << ", \"llr_off\": " << llr_off << ", \"nof_bits\": " << cw.used
       << ", \"sinr_db\": " << (std::isinf(stats.sinr) ? "\"inf\"" : t) << "}" << (ci + 1 == cases.size() ? "\n" : ",\n");
  }
  js << "]\n";
  write_npy(dir + "/pusch_tp_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pusch_tp_reference_ce.npy", "<u4", ces, 0);
  write_npy(dir + "/pusch_tp_reference_eq.npy", "<f4", eqs, 2);
  write_npy(dir + "/pusch_tp_reference_nvar.npy", "<f4", nvars, 0);
  write_npy(dir + "/pusch_tp_reference_z.npy", "<f4", zs, 2);
  write_npy(dir + "/pusch_tp_reference_llr.npy", "|i1", llrs, 0);
  std::fprintf(stderr, "%zu cases\n", cases.size());
  return 0;
}
