// Records the answers of srsRAN-5G-ER's srs_estimator_generic_impl for tests/test_srs_estimator.py.  It constructs the reference's
// classes directly -- the estimator with low_papr_sequence_generator_impl and time_alignment_estimator_dft_impl over
// dft_processor_generic_impl --, makes a grid per case with a transmitter of its own, and writes inputs and outputs as four .npy
// files.  Built and run by oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/:
// `make -C oracle recorders`, `make -C oracle rerecord-check`; no binary or object is committed.  The run takes several minutes:
// channels are drawn again, see below.
//
// -ffp-contract=off (the recipe's avx2nc flags): the estimator's phase index is a chain of single-precision operations in the
// source, and the recording holds what the source says; the compiler's default would fuse n * ps + offset wherever the target has a
// fused multiply-add.
//
// Cases: the 72 configurations of srs_configs.json ("estimator"), each with a seeded channel, then the small shapes of the table
// below.  Per case the transmitter puts antenna port p's sequence (the reference generator's) on its comb, gives receive port i
// the gain g[i][p] (amplitude 0.5..1.5, any phase) and the phase exp(-j 2 pi k d / 4096) of a delay of d bins on subcarrier k, adds
// complex Gaussian noise of standard deviation `noise` to every element of the SRS symbols and rounds to cbf16 (nearest, ties to
// even).  A channel whose searched bins hold two largest magnitudes within 2e-4 of each other on any path is drawn again (short
// sequences have flat peaks, and the other antenna ports tilt them): no recorded path is near a tie between two bins.
//
// Files (case i is row i of `cases` and of `results`):
//   srs_reference_cases.npy      int32 [n][28]: numerology, nof_antenna_ports, nof_symbols, start_symbol, configuration_index,
//                                sequence_id, bandwidth_index, comb_size, comb_offset, cyclic_shift, freq_position, freq_shift,
//                                freq_hopping, nof_rx_ports, rx_ports[4], grid_nof_ports, grid_nof_subc, delay d, noise in 1e-4,
//                                first stored subcarrier k_lo, stride s, stored subcarriers per row c, offset into grids, 0, 0
//   srs_reference_grids.npy      uint32 cbf16 words (re in the low half), the SRS symbols only: per case [grid_nof_ports][nof_symbols][c],
//                                element j the subcarrier k_lo + s j (s = comb, or comb / 2 where antenna ports sit on two combs);
//                                every other element of the case's grid is zero
//   srs_reference_results.npy    float64 [n][52]: h_re[4][4], h_im[4][4] ([rx][tx], zeros beyond the ports), the time alignment
//                                of every path in seconds [4][4] (what the reference's time alignment estimator returned to the
//                                estimator, through a forwarding wrapper), then time_alignment, min, max, resolution of the result
//   srs_reference_sequences.npy  float32 pairs: per distinct (u, M, n_cs, n_cs_max) of the cases the pairs (u, M), (n_cs, n_cs_max)
//                                and then the M values of low_papr_sequence_generator_impl::generate
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.h"
#include "recorder_grid.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_configuration.h"
#include "srsran/phy/upper/signal_processors/srs/srs_estimator_result.h"
#include "srsran/ran/srs/srs_information.h"

#include <cmath>
#include <complex>
#include <random>
#include <set>

using namespace srsran;

namespace {

// Forwards to the reference's estimator and keeps what it returned, call by call.  It also evaluates the searched bins of the
// call's symbols in double and says whether the two largest magnitudes lie within 2e-4 of each other: such a channel is drawn again.
class ta_recorder : public time_alignment_estimator
{
  std::unique_ptr<time_alignment_estimator> inner;
  std::vector<double>&                      log;
  bool&                                     near_tie;

  void look(span<const cf_t> symbols, unsigned stride, subcarrier_spacing scs, double max_ta)
  {
    const unsigned window = static_cast<unsigned>(std::floor(max_ta * static_cast<double>(scs_to_khz(scs) * 1000 * 4096)));
    double         top[2] = {0.0, 0.0};
    for (unsigned j = 0; j != 2 * window; ++j) {
      const unsigned       b = j < window ? j : 4096 - 2 * window + j;
      std::complex<double> x = 0.0;
      for (unsigned n = 0; n != symbols.size(); ++n) {
        const unsigned i = (stride * n * b) & 4095U;
        x += std::complex<double>(symbols[n].real(), symbols[n].imag()) * std::polar(1.0, 2.0 * M_PI * (double)i / 4096.0);
      }
      const double m = std::norm(x);
      if (m > top[0]) {
        top[1] = top[0];
        top[0] = m;
      } else if (m > top[1]) {
        top[1] = m;
      }
    }
    near_tie = near_tie || (top[0] - top[1] <= 2e-4 * top[0]);
  }

public:
  ta_recorder(std::unique_ptr<time_alignment_estimator> inner_, std::vector<double>& log_, bool& near_tie_) :
    inner(std::move(inner_)), log(log_), near_tie(near_tie_)
  {
  }
  time_alignment_measurement estimate(span<const cf_t> symbols, bounded_bitset<max_nof_symbols> mask, subcarrier_spacing scs, double max_ta) override
  {
    return inner->estimate(symbols, mask, scs, max_ta);
  }
  time_alignment_measurement estimate(span<const cf_t> symbols, unsigned stride, subcarrier_spacing scs, double max_ta) override
  {
    const time_alignment_measurement m = inner->estimate(symbols, stride, scs, max_ta);
    log.push_back(m.time_alignment);
    look(symbols, stride, scs, max_ta);
    return m;
  }
};

struct Case {
  int numerology, ntx, nsym, start, c_srs, seq_id, b_srs, comb, comb_offset, cs, fpos, fshift, fhop;
  std::vector<int> rx;
  int grid_ports, grid_subc, delay, noise; // noise in 1e-4
};

srs_estimator_configuration to_config(const Case& c)
{
  srs_estimator_configuration cfg;
  cfg.slot                         = slot_point(c.numerology, 0, 0, 0);
  cfg.resource.nof_antenna_ports   = srs_resource_configuration::one_two_four_enum(c.ntx);
  cfg.resource.nof_symbols         = srs_resource_configuration::one_two_four_enum(c.nsym);
  cfg.resource.start_symbol        = c.start;
  cfg.resource.configuration_index = c.c_srs;
  cfg.resource.sequence_id         = c.seq_id;
  cfg.resource.bandwidth_index     = c.b_srs;
  cfg.resource.comb_size           = srs_resource_configuration::comb_size_enum(c.comb);
  cfg.resource.comb_offset         = c.comb_offset;
  cfg.resource.cyclic_shift        = c.cs;
  cfg.resource.freq_position       = c.fpos;
  cfg.resource.freq_shift          = c.fshift;
  cfg.resource.freq_hopping        = c.fhop;
  cfg.resource.hopping             = srs_resource_configuration::group_or_sequence_hopping_enum::neither;
  for (int p : c.rx) {
    cfg.ports.push_back((uint8_t)p);
  }
  return cfg;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s srs_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream     in(argv[1]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  std::string text = buffer.str();
  text             = text.substr(0, text.find("\"validator\""));
  const std::string dir = argv[2];

  std::mt19937       rng(20240412);
  std::vector<Case>  cases;
  const std::regex   object("\\{\"numerology\"[^}]*\\}");
  for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it) {
    const std::string o = it->str();
    Case c = {json_int(o, "numerology"), json_int(o, "nof_antenna_ports"), json_int(o, "nof_symbols"), json_int(o, "start_symbol"),
              json_int(o, "configuration_index"), json_int(o, "sequence_id"), json_int(o, "bandwidth_index"), json_int(o, "comb_size"),
              json_int(o, "comb_offset"), json_int(o, "cyclic_shift"), json_int(o, "freq_position"), json_int(o, "freq_shift"),
              json_int(o, "freq_hopping"), json_list(o, "rx_ports"), 0, 0, 0, 500};
    c.grid_ports = c.rx.back() + 1;
    // A delay within half the search window of the comb: 256 bins for comb 2, 85 for comb 4.
    const int w = c.comb == 2 ? 256 : 85;
    c.delay     = (int)(rng() % (unsigned)w) - w / 2;
    cases.push_back(c);
  }
  const size_t nof_reference = cases.size();
  // The small shapes: {numerology, ports, symbols, start, C_SRS, id, B_SRS, comb, offset, shift, n_RRC, n_shift, b_hop}, rx ports,
  // grid ports, grid subcarriers, delay, noise.
  const std::vector<Case> small = {
      {0, 1, 1, 13, 0, 7, 0, 4, 2, 0, 0, 0, 3, {2}, 4, 624, 0, 500},             // M 12
      {1, 2, 2, 12, 0, 41, 0, 2, 1, 3, 0, 1, 3, {1, 0}, 4, 624, 3, 500},          // M 24, comb 2
      {0, 4, 4, 10, 1, 100, 0, 4, 0, 2, 0, 0, 3, {3, 1, 0, 2}, 4, 624, -3, 500},  // M 24, comb 4, four ports, no comb swap
      {1, 4, 1, 13, 2, 512, 0, 4, 1, 7, 0, 2, 3, {0, 1}, 4, 624, 3, 500},         // M 36, four ports, comb swap
      {0, 4, 2, 12, 1, 29, 0, 2, 0, 5, 0, 0, 3, {2, 3, 1}, 4, 624, -3, 500},      // M 48, four ports, comb swap
      {0, 4, 1, 13, 1, 1023, 0, 2, 1, 1, 0, 3, 3, {0, 1, 2, 3}, 4, 624, 0, 500},  // M 48, four ports, no comb swap
      {0, 1, 1, 13, 14, 3, 0, 2, 0, 0, 0, 0, 3, {0}, 4, 624, 255, 500},           // M 312, delay W - 1
      {1, 2, 4, 10, 14, 64, 0, 2, 1, 2, 0, 0, 3, {3, 0}, 4, 624, -256, 500},      // M 312, delay -W
      {0, 1, 2, 12, 14, 5, 0, 4, 3, 0, 0, 0, 3, {1}, 4, 624, 84, 500},            // M 156, comb 4, delay W - 1
      {1, 2, 1, 13, 14, 77, 0, 4, 1, 4, 0, 0, 3, {0, 2}, 4, 624, -85, 500},       // M 156, comb 4, delay -W
      {0, 2, 1, 13, 14, 330, 1, 2, 0, 6, 5, 3, 3, {1, 2}, 4, 624, 3, 500},        // B_SRS 1, n_RRC 5, n_shift 3
      {1, 1, 2, 12, 9, 17, 2, 4, 2, 11, 3, 2, 2, {0, 3}, 4, 624, -3, 500},        // B_SRS 2, n_RRC 3, n_shift 2
      {1, 4, 1, 13, 63, 901, 0, 2, 0, 6, 0, 0, 3, {0, 1, 2, 3}, 4, 3264, 3, 500}, // M 1632, 272 PRB
  };
  cases.insert(cases.end(), small.begin(), small.end());

  std::vector<double> ta_log;
  bool                near_tie = false;
  dft_processor::configuration dft_cfg;
  dft_cfg.size = 4096;
  dft_cfg.dir  = dft_processor::direction::INVERSE;
  srs_estimator_generic_impl::dependencies deps;
  deps.sequence_generator = std::make_unique<low_papr_sequence_generator_impl>();
  deps.ta_estimator       = std::make_unique<ta_recorder>(
      std::make_unique<time_alignment_estimator_dft_impl>(std::make_unique<dft_processor_generic_impl>(dft_cfg)), ta_log, near_tie);
  srs_estimator_generic_impl       estimator(std::move(deps));
  low_papr_sequence_generator_impl generator;

  std::vector<int32_t>              rows;
  std::vector<uint32_t>             grids;
  std::vector<double>               results;
  std::vector<float>                sequences;
  std::set<std::vector<unsigned>>   seen;
  std::normal_distribution<float>   normal(0.0F, 1.0F);
  std::uniform_real_distribution<float> uniform(0.0F, 1.0F);
  for (size_t ic = 0; ic != cases.size(); ++ic) {
    Case&                             c   = cases[ic];
    const srs_estimator_configuration cfg = to_config(c);
    // The grid: as many subcarriers as the SRS needs, in whole PRBs (the small shapes say theirs).
    unsigned k_lo = ~0U, k_hi = 0;
    bool     two_combs = false;
    for (int p = 0; p != c.ntx; ++p) {
      const srs_information info = get_srs_information(cfg.resource, p);
      k_lo      = std::min(k_lo, info.mapping_initial_subcarrier);
      k_hi      = std::max(k_hi, info.mapping_initial_subcarrier + info.comb_size * (info.sequence_length - 1));
      two_combs = two_combs || (info.mapping_initial_subcarrier % c.comb != get_srs_information(cfg.resource, 0).mapping_initial_subcarrier % c.comb);
    }
    if (ic < nof_reference) {
      c.grid_subc = 12 * (k_hi / 12 + 1);
    }
    if (k_hi >= (unsigned)c.grid_subc) {
      std::fprintf(stderr, "case %zu does not fit its grid\n", ic);
      return 1;
    }
    word_grid            grid(c.grid_ports, c.grid_subc);
    srs_estimator_result r;
    unsigned             attempts = 0;
    do { // a channel, until no path is near a tie
      std::vector<std::vector<cf_t>> acc(c.grid_ports, std::vector<cf_t>(c.grid_subc, cf_t(0, 0)));
      for (int p = 0; p != c.ntx; ++p) {
        const srs_information info = get_srs_information(cfg.resource, p);
        std::vector<cf_t>     seq(info.sequence_length);
        generator.generate(seq, info.sequence_group, info.sequence_number, info.n_cs, info.n_cs_max);
        const std::vector<unsigned> key = {info.sequence_group, info.sequence_length, info.n_cs, info.n_cs_max};
        if (seen.insert(key).second) {
          for (unsigned v : key) {
            sequences.push_back((float)v);
          }
          for (const cf_t& v : seq) {
            sequences.push_back(v.real());
            sequences.push_back(v.imag());
          }
        }
        for (int i : c.rx) {
          const float  amplitude = 0.5F + uniform(rng), angle = 6.2831853F * uniform(rng);
          const std::complex<double> g = std::polar((double)amplitude, (double)angle);
          for (unsigned n = 0; n != info.sequence_length; ++n) {
            const unsigned k = info.mapping_initial_subcarrier + info.comb_size * n;
            const std::complex<double> v = g * std::complex<double>(seq[n].real(), seq[n].imag()) *
                                           std::polar(1.0, -2.0 * M_PI * (double)k * (double)c.delay / 4096.0);
            acc[i][k] += cf_t((float)v.real(), (float)v.imag());
          }
        }
      }
      const float sigma = (float)c.noise * 1e-4F * std::sqrt(0.5F);
      for (int port = 0; port != c.grid_ports; ++port) {
        for (int l = c.start; l != c.start + c.nsym; ++l) {
          for (int k = 0; k != c.grid_subc; ++k) {
            grid.set(port, l, k, acc[port][k].real() + sigma * normal(rng), acc[port][k].imag() + sigma * normal(rng));
          }
        }
      }
      ta_log.clear();
      near_tie = false;
      r        = estimator.estimate(grid, cfg);
    } while (near_tie && ++attempts != 100000);
    if (near_tie) {
      std::fprintf(stderr, "case %zu: every channel near a tie\n", ic);
      return 1;
    }
    if (ta_log.size() != (size_t)c.ntx * c.rx.size()) {
      std::fprintf(stderr, "case %zu: %zu time alignment calls\n", ic, ta_log.size());
      return 1;
    }
    const unsigned stride = two_combs ? c.comb / 2 : c.comb, count = (k_hi - k_lo) / stride + 1;
    const int32_t  row[28] = {c.numerology, c.ntx, c.nsym, c.start, c.c_srs, c.seq_id, c.b_srs, c.comb, c.comb_offset, c.cs, c.fpos, c.fshift,
                              c.fhop, (int)c.rx.size(), c.rx[0], c.rx.size() > 1 ? c.rx[1] : 0, c.rx.size() > 2 ? c.rx[2] : 0,
                              c.rx.size() > 3 ? c.rx[3] : 0, c.grid_ports, c.grid_subc, c.delay, c.noise, (int)k_lo, (int)stride, (int)count,
                              (int)grids.size(), 0, 0};
    rows.insert(rows.end(), row, row + 28);
    for (int port = 0; port != c.grid_ports; ++port) {
      for (int l = c.start; l != c.start + c.nsym; ++l) {
        for (unsigned j = 0; j != count; ++j) {
          grids.push_back(grid.word(port, l, k_lo + stride * j));
        }
      }
    }
    double out[52] = {};
    for (unsigned i = 0; i != c.rx.size(); ++i) {
      for (int p = 0; p != c.ntx; ++p) {
        const cf_t h       = r.channel_matrix.get_coefficient(i, p);
        out[4 * i + p]      = h.real();
        out[16 + 4 * i + p] = h.imag();
        out[32 + 4 * i + p] = ta_log[(size_t)p * c.rx.size() + i]; // the estimator calls antenna port outer, receive port inner
      }
    }
    out[48] = r.time_alignment.time_alignment;
    out[49] = r.time_alignment.min;
    out[50] = r.time_alignment.max;
    out[51] = r.time_alignment.resolution;
    results.insert(results.end(), out, out + 52);
  }
  write_npy(dir + "/srs_reference_cases.npy", "<i4", rows, 28);
  write_npy(dir + "/srs_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/srs_reference_results.npy", "<f8", results, 52);
  write_npy(dir + "/srs_reference_sequences.npy", "<f4", sequences, 0);
  std::printf("%zu cases (%zu of the reference's), %zu grid words, %zu sequence floats\n", cases.size(), nof_reference, grids.size(), sequences.size());
  return 0;
}
