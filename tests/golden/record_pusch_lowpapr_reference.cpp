// Records the answers of srsRAN-5G-ER's port channel estimator on the low-PAPR DM-RS of a transform-precoded PUSCH, for
// tests/test_pusch_lowpapr.py.  The reference's dmrs_pusch_estimator_impl generates Gold-sequence pilots only; its later releases
// feed low_papr_sequence_generator::generate(seq, n_rs_id % 30, 0, 0, 1) into the unchanged port_channel_estimator.  This
// recorder does the same with the two classes of this checkout: it drives low_papr_sequence_generator_impl and
// port_channel_estimator_average_impl (`filter` smoothing, compensate_cfo = true, interpolator_linear_impl and
// time_alignment_estimator_dft_impl over a 4096-point inverse dft_processor_generic_impl, as signal_processor_factories.cpp does
// for PUSCH) directly, and lays out pilots and pattern as dmrs_pusch_estimator_impl::estimate does for one layer of DM-RS type 1:
// the same sequence on every DM-RS symbol, symbols and PRBs of the allocation, RE pattern delta 0.  Then the DC step of
// pusch_processor_impl.cpp:182-199 where the case names a DC subcarrier.
//
// The generator builds its exponential tables for the SRS lengths only (its `sequence_sizes`); a PUSCH DM-RS has 6 M_rb pilots,
// M_rb = 2^a 3^b 5^c, and most of those lengths need a table of 2 N_zc entries that the constructor did not make.  The recorder
// adds the missing ones, each a complex_exponential_table(2 N_zc, 1.0) -- the reference's own class and arguments -- into the
// generator's private map: hence -fno-access-control.  M_rb = 5 (30 pilots) is a length the generator terminates on; nothing of
// that size is recorded.
//
// Built and run by oracle/recorders.mk from command-line variables, against a checkout of srsRAN-5G-ER and into oracle/_ref/;
// no binary or object is committed:
//   make -C oracle rerecord-pusch_lowpapr RECORDERS=pusch_lowpapr SELF_CONTAINED=pusch_lowpapr FLAVOUR_pusch_lowpapr=avx2nc \
//     'SRCS_pusch_lowpapr=$(U)/sequence_generators/low_papr_sequence_generator_impl.cpp $(CHEST) $(FMT)' \
//     OWN_pusch_lowpapr=-fno-access-control 'ARGS_pusch_lowpapr=$(RECORDED)'
// The flags are those of record_pusch_chest_reference.cpp.
//
// The forwarding interpolator and time alignment estimator, the transmitter and channel, and the rule against fragile time
// alignment decisions (a lead of min(2 %, c / 2) over the runner-up, in double) are record_pusch_chest_reference.cpp's; see
// there.  The transmitter sends beta x the low-PAPR sequence on the pilots of every DM-RS symbol.
//
// Files (offsets in elements of the named file):
//   pusch_lowpapr_reference_cases.json     per case: name, numerology, n_rs_id, scaling, dmrs_symbols, first_symbol, nof_symbols,
//                                          rx_ports, prbs (grid PRB numbers), grid_prb, dc (grid subcarrier, -1: none), snr_db,
//                                          delay (with the drawn fraction), cfo_hz, draws, grid_off, pilot_off, est_off, res_row
//   pusch_lowpapr_reference_grids.npy      uint32 cbf16 words (re in the low half): per case [P][nof_dmrs][12 nprb], row i what
//                                          receive port i reads (grid port rx_ports[i])
//   pusch_lowpapr_reference_pilots.npy     complex64: per case [P][6 nprb], the smoothed pilots
//   pusch_lowpapr_reference_estimates.npy  uint32 cbf16 words: per case [P][nof_symbols][12 nprb], the estimate on the allocated
//                                          PRBs of symbols first_symbol ..., after the DC step
//   pusch_lowpapr_reference_results.npy    float64 [rows][12], row res_row + port: the columns of
//                                          pusch_chest_reference_results.npy
//   pusch_lowpapr_reference_sequences.npy  complex64: generate(u, 0, 0, 1) of length 6 M_rb, for u = 0 and u = 29 (in this
//                                          order) of every valid M_rb but 5 in ascending order; then, for the table sizes
//                                          M_rb = 1, 2, 3, 4 in this order, u = 0 .. 29 (what the phi tables are read from)
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "recorder_grid.h"
#include "srsran/ran/transform_precoding/transform_precoding_helpers.h"
#include "srsran/support/math_utils.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>
#include <random>

using namespace srsran;

namespace {

constexpr double MARGIN = 0.02;
constexpr int    TA_WINDOW = 144, DFT = 4096;
const double     NaN = std::numeric_limits<double>::quiet_NaN();
using cd = std::complex<double>;

// Forwards to the reference's interpolator and keeps the input of every call.
class interpolator_recorder : public interpolator
{
  std::unique_ptr<interpolator>   inner;
  std::vector<std::vector<cf_t>>& log;

public:
  interpolator_recorder(std::unique_ptr<interpolator> inner_, std::vector<std::vector<cf_t>>& log_) : inner(std::move(inner_)), log(log_) {}
  void interpolate(span<cf_t> output, span<const cf_t> input, const configuration& cfg) override
  {
    if (cfg.offset != 0 || cfg.stride != 2) {
      std::fprintf(stderr, "interpolator: offset %u stride %u\n", cfg.offset, cfg.stride);
      std::exit(1);
    }
    log.emplace_back(input.begin(), input.end());
    inner->interpolate(output, input, cfg);
  }
};

// Forwards to the reference's time alignment estimator and keeps what it was handed and what it answered, call by call.
struct ta_call {
  std::vector<cf_t>     symbols;
  std::vector<unsigned> subc;
  unsigned              scs_khz;
  double                answer;
};
class ta_recorder : public time_alignment_estimator
{
  std::unique_ptr<time_alignment_estimator> inner;
  std::vector<ta_call>&                     log;

public:
  ta_recorder(std::unique_ptr<time_alignment_estimator> inner_, std::vector<ta_call>& log_) : inner(std::move(inner_)), log(log_) {}
  time_alignment_measurement estimate(span<const cf_t> symbols, bounded_bitset<max_nof_symbols> mask, subcarrier_spacing scs, double max_ta) override
  {
    ta_call c;
    c.symbols.assign(symbols.begin(), symbols.end());
    for (unsigned i = 0; i != mask.size(); ++i) {
      if (mask.test(i)) {
        c.subc.push_back(i);
      }
    }
    c.scs_khz = scs_to_khz(scs);
    if (max_ta != 0.0) {
      std::fprintf(stderr, "time alignment: max_ta %g\n", max_ta);
      std::exit(1);
    }
    const time_alignment_measurement m = inner->estimate(symbols, mask, scs, max_ta);
    c.answer                           = m.time_alignment;
    log.push_back(c);
    return m;
  }
  time_alignment_measurement estimate(span<const cf_t>, unsigned, subcarrier_spacing, double) override
  {
    std::fprintf(stderr, "time alignment: the strided call is not the PUSCH estimator's\n");
    std::exit(1);
  }
};

struct Case {
  std::string      name;
  int              numerology, n_rs_id;
  float            scaling;
  std::vector<int> dmrs;
  int              start, ns;
  std::vector<int> ports, prbs;
  int              grid_prb, dc;
  double           snr_db, delay, cfo_hz;
};

// name, numerology, n_rs_id, beta, DM-RS symbols, first symbol, symbols, rx ports, PRBs, grid PRBs, DC, SNR, delay, CFO.  Each is
// the smallest shape at which one branch of the sequence or of the kernel is first taken.
std::vector<Case> cases_list()
{
  const float b3 = 1.4125F; // two CDM groups without data: what the processor hands down
  return {
      // the four tables; one DM-RS symbol has no CFO
      {"1 PRB (length 6), 1 DM-RS, n_rs_id 0", 0, 0, 1.0F, {2}, 0, 14, {0}, {7}, 52, -1, 20, 3, 150},
      {"2 PRB (length 12), 2 DM-RS, n_rs_id 29, ports (1, 0)", 0, 29, b3, {2, 11}, 0, 14, {1, 0}, {10, 11}, 52, -1, 20, 1, -200},
      {"3 PRB (length 18), 3 DM-RS, n_rs_id 30, 3 ports", 0, 30, b3, {2, 7, 11}, 0, 14, {0, 1, 2}, {20, 21, 22}, 52, -1, 20, -2, 250},
      {"4 PRB (length 24), 4 DM-RS, mu 1, n_rs_id 1007, ports (3, 1, 0, 2), window 1..13", 1, 1007, b3, {2, 5, 8, 11}, 1, 13, {3, 1, 0, 2},
       range(30, 4), 52, -1, 20, 3, -300},
      // the first Zadoff-Chu size: N_zc = 31, pilots 31 .. 35 wrap
      {"6 PRB (N_zc 31), 2 DM-RS, n_rs_id 17", 0, 17, b3, {2, 11}, 0, 14, {0}, range(3, 6), 52, -1, 20, 2, 100},
      // a scatter of PRBs with DC inside one of them
      {"8 PRB: 0, 2, 4, 6, 8-11, DC in PRB 4, n_rs_id 400", 0, 400, b3, {3, 10}, 2, 12, {0, 1}, {0, 2, 4, 6, 8, 9, 10, 11}, 52, 12 * 4 + 6, 20, -3,
       200},
      {"25 PRB, DC in the middle, n_rs_id 1007, 2 ports", 0, 1007, b3, {2, 11}, 0, 14, {0, 1}, range(13, 25), 52, 12 * 26, 20, 2, -100},
      {"25 PRB at 0 dB, n_rs_id 30", 0, 30, b3, {2, 7, 11}, 0, 14, {0}, range(13, 25), 52, -1, 0, -40, 100},
      // 1620 pilots: q m (m + 1) needs 64 bits
      {"270 PRB, 2 DM-RS, n_rs_id 29, window 2..11", 0, 29, b3, {2, 11}, 2, 10, {0}, range(2, 270), 273, -1, 20, 3, 150},
  };
}

struct PathResult {
  double row[12];
};

struct Reference {
  std::vector<std::vector<cf_t>>                       smoothed;
  std::vector<ta_call>                                 ta_log;
  std::unique_ptr<port_channel_estimator_average_impl> estimator;
  low_papr_sequence_generator_impl                     generator;
  std::unique_ptr<dmrs_symbol_list>                    pilots = std::make_unique<dmrs_symbol_list>();
  channel_estimate                                     estimate;

  Reference()
  {
    dft_processor::configuration dft_cfg;
    dft_cfg.size = DFT;
    dft_cfg.dir  = dft_processor::direction::INVERSE;
    estimator    = std::make_unique<port_channel_estimator_average_impl>(
        std::make_unique<interpolator_recorder>(std::make_unique<interpolator_linear_impl>(), smoothed),
        std::make_unique<ta_recorder>(
            std::make_unique<time_alignment_estimator_dft_impl>(std::make_unique<dft_processor_generic_impl>(dft_cfg)), ta_log),
        port_channel_estimator_fd_smoothing_strategy::filter,
        /*compensate_cfo =*/true);
    // The tables of the lengths the constructor did not foresee (see the header comment).
    for (unsigned nprb = 6; nprb <= 275; ++nprb) {
      const unsigned size = 2 * prime_lower_than(6 * nprb);
      if (is_transform_precoding_nof_prb_valid(nprb) && generator.tables.count(size) == 0) {
        generator.tables.emplace(size, complex_exponential_table(size, 1.0));
      }
    }
    if (generator.temp_r_uv_arg.size() < 6 * 270) {
      std::fprintf(stderr, "the generator's temporaries hold %zu\n", generator.temp_r_uv_arg.size());
      std::exit(1);
    }
  }

  // low_papr_sequence_generator::generate(seq, n_rs_id % 30, 0, 0, 1): group and sequence hopping off.
  std::vector<cf_t> sequence(unsigned u, unsigned nprb)
  {
    std::vector<cf_t> out(6 * nprb);
    generator.generate(out, u, 0, 0, 1);
    return out;
  }

  void run(const word_grid& grid, const Case& c, const std::vector<cf_t>& seq)
  {
    const unsigned            P = c.ports.size();
    re_measurement_dimensions dims;
    dims.nof_subc    = seq.size();
    dims.nof_symbols = c.dmrs.size();
    dims.nof_slices  = 1;
    pilots->resize(dims);
    for (unsigned dd = 0; dd != c.dmrs.size(); ++dd) {
      span<cf_t> dst = pilots->get_symbol(dd, 0);
      std::copy(seq.begin(), seq.end(), dst.begin());
    }
    port_channel_estimator::layer_dmrs_pattern pattern;
    pattern.symbols = bounded_bitset<MAX_NSYMB_PER_SLOT>(14);
    for (int l : c.dmrs) {
      pattern.symbols.set(l);
    }
    pattern.rb_mask = bounded_bitset<MAX_RB>(c.grid_prb);
    for (int n : c.prbs) {
      pattern.rb_mask.set(n);
    }
    pattern.re_pattern = {true, false, true, false, true, false, true, false, true, false, true, false}; // type 1, delta 0
    port_channel_estimator::configuration e;
    e.scs          = to_subcarrier_spacing(c.numerology);
    e.cp           = cyclic_prefix::NORMAL;
    e.first_symbol = c.start;
    e.nof_symbols  = c.ns;
    e.dmrs_pattern.push_back(pattern);
    e.scaling = c.scaling;
    for (unsigned i = 0; i != P; ++i) {
      e.rx_ports.push_back((uint8_t)i);
    }
    estimate.resize({(unsigned)c.grid_prb, (unsigned)(c.start + c.ns), P, 1U});
    const cbf16_t untouched(7.0F, -7.0F);
    for (unsigned i = 0; i != P; ++i) {
      span<cbf16_t> path = estimate.get_path_ch_estimate(i, 0);
      std::fill(path.begin(), path.end(), untouched);
    }
    smoothed.clear();
    ta_log.clear();
    for (unsigned i = 0; i != P; ++i) {
      estimator->compute(estimate, grid, i, *pilots, e);
    }
  }
};

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 1;
  }
  const std::string dir = argv[1];
  Reference         ref;

  // ---- the sequences ----
  std::vector<cf_t> sequences;
  unsigned          nof_sizes = 0;
  for (unsigned nprb = 1; nprb <= 275; ++nprb) {
    if (!is_transform_precoding_nof_prb_valid(nprb) || nprb == 5) {
      continue;
    }
    ++nof_sizes;
    for (unsigned u : {0U, 29U}) {
      const std::vector<cf_t> s = ref.sequence(u, nprb);
      sequences.insert(sequences.end(), s.begin(), s.end());
    }
  }
  for (unsigned nprb = 1; nprb <= 4; ++nprb) {
    for (unsigned u = 0; u != 30; ++u) {
      const std::vector<cf_t> s = ref.sequence(u, nprb);
      sequences.insert(sequences.end(), s.begin(), s.end());
    }
  }
  write_npy(dir + "/pusch_lowpapr_reference_sequences.npy", "<c8", sequences, 0);
  std::printf("%u sizes, %zu sequence elements\n", nof_sizes, sequences.size());

  // ---- the estimator ----
  const std::vector<Case>                cases = cases_list();
  std::mt19937                           rng(20261021);
  std::normal_distribution<double>       normal(0.0, 1.0);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  std::vector<uint32_t>                  grids, estimates;
  std::vector<cf_t>                      pilots;
  std::vector<double>                    results;
  std::ostringstream                     json;
  size_t                                 draws_total = 0;
  json << "[\n";
  for (size_t ic = 0; ic != cases.size(); ++ic) {
    const Case&               c = cases[ic];
    const unsigned            P = c.ports.size(), nprb = c.prbs.size(), N = 6 * nprb, nd = c.dmrs.size();
    const std::vector<double> ep = epochs(c.numerology);
    const double              scs = 15000.0 * (1 << c.numerology);
    std::vector<unsigned>     subc; // the allocation's subcarriers, ascending
    for (int n : c.prbs) {
      for (unsigned k = 0; k != 12; ++k) {
        subc.push_back(12 * n + k);
      }
    }
    double mean = 0.0, var = 0.0;
    for (unsigned q = 0; q != N; ++q) {
      mean += subc[2 * q] / (double)N;
    }
    for (unsigned q = 0; q != N; ++q) {
      var += (subc[2 * q] - mean) * (subc[2 * q] - mean) / N;
    }
    const double asked = std::min(MARGIN, 0.5 * (2 * M_PI / DFT) * (2 * M_PI / DFT) * var);

    const std::vector<cf_t> tx = ref.sequence(c.n_rs_id % 30, nprb);
    word_grid               grid(P, 12 * c.grid_prb);
    std::vector<PathResult> res(P);
    unsigned                draws = 0;
    double                  delay = c.delay;
    bool                    fragile;
    do {
      ++draws;
      delay = c.delay + uniform(rng) - 0.5;
      const double sigma = std::sqrt(std::pow(10.0, -c.snr_db / 10.0) / 2); // per component
      for (unsigned p = 0; p != P; ++p) {
        const cd g0 = std::polar(1.0, 2 * M_PI * uniform(rng)), g1 = std::polar(0.5, 2 * M_PI * uniform(rng));
        for (unsigned dd = 0; dd != nd; ++dd) {
          const cd rot = std::polar(1.0, 2 * M_PI * (c.cfo_hz / scs) * ep[c.dmrs[dd]]);
          for (unsigned j = 0; j != 12 * nprb; ++j) {
            cd v = 0.0;
            if (j % 2 == 0) {
              const double k = subc[j];
              const cd     h = g0 * std::polar(1.0, -2 * M_PI * k * delay / DFT) + g1 * std::polar(1.0, -2 * M_PI * k * (delay + 4) / DFT);
              v              = h * (double)c.scaling * cd(tx[j / 2].real(), tx[j / 2].imag());
            }
            v = v * rot + sigma * cd(normal(rng), normal(rng));
            grid.set(p, c.dmrs[dd], subc[j], (float)v.real(), (float)v.imag());
          }
        }
      }
      ref.run(grid, c, tx);
      if (ref.smoothed.size() != P || ref.ta_log.size() != P) {
        std::fprintf(stderr, "case %zu: %zu interpolations and %zu time alignments for %u ports\n", ic, ref.smoothed.size(), ref.ta_log.size(), P);
        return 1;
      }
      fragile = false;
      for (unsigned p = 0; p != P; ++p) {
        const std::vector<cf_t>& f  = ref.smoothed[p];
        const ta_call&           ta = ref.ta_log[p];
        bool                     same = f.size() == N && ta.symbols.size() == N && ta.subc.size() == N && ta.scs_khz * 1000.0 == scs;
        for (unsigned q = 0; same && q != N; ++q) {
          same = std::memcmp(&f[q], &ta.symbols[q], sizeof(cf_t)) == 0 && ta.subc[q] == subc[2 * q];
        }
        if (!same) {
          std::fprintf(stderr, "case %zu: the time alignment estimator was not handed the smoothed pilots\n", ic);
          return 1;
        }
        double best = -1.0, second = -1.0;
        int    best_bin = 0;
        for (int b = -TA_WINDOW; b != TA_WINDOW; ++b) {
          cd x = 0.0;
          for (unsigned q = 0; q != N; ++q) {
            x += cd(f[q].real(), f[q].imag()) * std::polar(1.0, 2 * M_PI * (double)b * subc[2 * q] / DFT);
          }
          const double pw = std::norm(x);
          if (pw > best) {
            second   = best;
            best     = pw;
            best_bin = b;
          } else if (pw > second) {
            second = pw;
          }
        }
        fragile              = fragile || (best - second < asked * best);
        const double bin     = ta.answer * DFT * scs;
        const double row[12] = {ref.estimate.get_noise_variance(p, 0), ref.estimate.get_rsrp(p, 0), ref.estimate.get_epre(p, 0),
                                ref.estimate.get_snr(p, 0), ref.estimate.get_time_alignment(p, 0).to_seconds(),
                                ref.estimate.get_cfo_Hz(p, 0).has_value() ? (double)ref.estimate.get_cfo_Hz(p, 0).value() : NaN,
                                ta.answer, std::round(bin), best, second, asked, 0.0};
        std::memcpy(res[p].row, row, sizeof(row));
        if (!fragile && (std::fabs(bin - std::round(bin)) > 1e-6 || (int)std::round(bin) != best_bin)) {
          std::fprintf(stderr, "case %zu port %u: the reference's bin %g, %d in double with a lead of %g\n", ic, p, bin, best_bin,
                       (best - second) / best);
          return 1;
        }
      }
    } while (fragile && draws != 10000);
    if (fragile) {
      std::fprintf(stderr, "case %zu (%s): every draw fragile\n", ic, c.name.c_str());
      return 1;
    }
    draws_total += draws;

    // The DC step of pusch_processor_impl.
    if (c.dc >= 0) {
      for (unsigned p = 0; p != P; ++p) {
        for (int s = c.start; s != c.start + c.ns; ++s) {
          span<cbf16_t> ce = ref.estimate.get_symbol_ch_estimate(s, p, 0);
          ce[c.dc]         = 0;
        }
      }
    }

    const size_t grid_off = grids.size(), pilot_off = pilots.size(), est_off = estimates.size(), res_row = results.size() / 12;
    for (unsigned p = 0; p != P; ++p) {
      for (int l : c.dmrs) {
        for (unsigned k : subc) {
          grids.push_back(grid.word(p, l, k));
        }
      }
      pilots.insert(pilots.end(), ref.smoothed[p].begin(), ref.smoothed[p].end());
      results.insert(results.end(), res[p].row, res[p].row + 12);
    }
    std::vector<bool> allocated(12 * c.grid_prb, false);
    for (unsigned k : subc) {
      allocated[k] = true;
    }
    for (unsigned p = 0; p != P; ++p) {
      for (int s = c.start; s != c.start + c.ns; ++s) {
        span<const cbf16_t> row = ref.estimate.get_symbol_ch_estimate(s, p, 0);
        for (unsigned k = 0; k != row.size(); ++k) {
          if (allocated[k]) {
            estimates.push_back(word_of(row[k]));
          }
        }
      }
    }
    char num[128];
    std::snprintf(num, sizeof(num), "\"scaling\": %.9g, \"snr_db\": %.17g, \"delay\": %.17g, \"cfo_hz\": %.17g", (double)c.scaling, c.snr_db, delay, c.cfo_hz);
    json << (ic ? ",\n" : "") << "{\"name\": \"" << c.name << "\", \"numerology\": " << c.numerology << ", \"n_rs_id\": " << c.n_rs_id << ", " << num
         << ", \"dmrs_symbols\": " << list_json(c.dmrs) << ", \"first_symbol\": " << c.start << ", \"nof_symbols\": " << c.ns
         << ", \"rx_ports\": " << list_json(c.ports) << ", \"prbs\": " << list_json(c.prbs) << ", \"grid_prb\": " << c.grid_prb << ", \"dc\": " << c.dc
         << ", \"draws\": " << draws << ", \"grid_off\": " << grid_off << ", \"pilot_off\": " << pilot_off << ", \"est_off\": " << est_off
         << ", \"res_row\": " << res_row << "}";
    std::printf("case %2zu: %u draws, lead asked %.3g  %s\n", ic, draws, asked, c.name.c_str());
  }
  json << "\n]\n";
  std::ofstream(dir + "/pusch_lowpapr_reference_cases.json") << json.str();
  write_npy(dir + "/pusch_lowpapr_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pusch_lowpapr_reference_pilots.npy", "<c8", pilots, 0);
  write_npy(dir + "/pusch_lowpapr_reference_estimates.npy", "<u4", estimates, 0);
  write_npy(dir + "/pusch_lowpapr_reference_results.npy", "<f8", results, 12);
  std::printf("%zu cases, %zu draws; %zu grid words, %zu pilots, %zu estimate words, %zu result rows\n", cases.size(), draws_total, grids.size(),
              pilots.size(), estimates.size(), results.size() / 12);
  return 0;
}
