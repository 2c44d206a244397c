// Records the answers of srsRAN-5G-ER's PUSCH DM-RS channel estimator for tests/test_pusch_channel_estimator.py.  It constructs
// dmrs_pusch_estimator_impl over port_channel_estimator_average_impl as signal_processor_factories.cpp does for PUSCH (`filter`
// smoothing, compensate_cfo = true), with interpolator_linear_impl and time_alignment_estimator_dft_impl over a 4096-point inverse
// dft_processor_generic_impl, makes a grid per case with a transmitter of its own, and writes inputs and outputs as one .json and
// four .npy files.  DM-RS type 1, one or two layers: what nrphy_pusch_chest_run supports.  Built and run by
// oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`,
// `make -C oracle rerecord-check`; no binary or object is committed.  The flags are those of the archive
// record_pusch_processor_reference.cpp links, so both recordings describe one build of the reference.
//
// The estimator is handed two forwarding objects.  The forwarding interpolator keeps its float32 input per (port, layer): the
// smoothed pilots, after LS, CFO derotation, averaging, virtual pilots and the FIR and before any bf16 rounding.  The forwarding
// time_alignment_estimator keeps what it was handed and what it answered; the recorder stops unless it was handed the smoothed
// pilots, bit for bit, on the allocation's pilot subcarriers.
//
// Receive ports: as in the other recorders the reference is handed the list 0 .. n - 1 and a grid whose port i is what receive
// port i reads.  The DC step is pusch_processor_impl's, not the estimator's: nothing here has it (NRPHY_PUSCH_CHEST_NO_DC).
//
// Transmitter and channel: those of synthetic_grid() in the test file.  On the DM-RS symbols layer l sends beta x its DM-RS (the
// reference's pseudo_random_generator_impl through dmrs_sequence_generate; layer 1 with the sign of port 1001 on the odd pilots)
// and nothing between the pilots; per (port, layer) two taps, e^{j phi} at `delay` and e^{j phi'} / 2 four samples later
// (samples of a 4096-point transform); a CFO as a phase per symbol start epoch; complex Gaussian noise of variance
// 10^(-snr_db / 10); every component rounded to bf16 (nearest, ties to even).  A case without a UE holds the noise alone.
//
// No fragile decision is recorded.  The only decision of this stage is the time alignment bin: the largest |x(n)|^2 of the 4096-
// point inverse transform of the smoothed pilots over n in [0, 144) and [3952, 4096).  For every (port, layer) the recorder
// evaluates those 288 powers in double and draws the case's delay fraction, channel and noise again while the best bin leads the
// runner-up, by (best - runner-up) / best, by less than
//     min(2 %, c / 2),  c = (2 pi / 4096)^2 Var(k),  Var(k) the variance of the allocation's pilot subcarrier numbers.
// 2 % is MARGIN of record_pucch_reference.cpp.  It cannot be asked of every shape: the transform of pilots that span few
// subcarriers is smooth, and around its peak a bin leads its neighbour by at most about c (a flat channel whose delay is a whole
// number of samples) -- 2.7e-5 for 1 PRB, 1.8 % for 25 PRB, above 2 % from 27 PRB on.  c / 2 keeps the peak within a quarter of
// a sample of its bin, and is 20 times what float32 rounding moves these powers by at 1 PRB (about 6e-7).  The recorder stops
// if the reference's bin is not the one found in double.
//
// Cases: small_shapes() below, each the smallest shape at which one branch of the library's kernel is first taken, then the type 1
// `ch_estimation` entries of pusch_chest_configs.json with at most 111 PRB (6 of 24; every further one would put the estimates
// above 1 MB), with the SNR, delay and CFO tests/test_pusch_channel_estimator.py::test_parity_with_the_restatement gives them.
//
// Files (offsets in elements of the named file):
//   pusch_chest_reference_cases.json     per case: name, numerology, slot_index, scrambling_id, n_scid, scaling, dmrs_symbols,
//                                        first_symbol, nof_symbols, nof_tx_layers, rx_ports, prbs (grid PRB numbers), grid_prb (width
//                                        of the grid in PRB), ue (0: noise only), snr_db, delay (with the drawn fraction), cfo_hz,
//                                        source (entry of pusch_chest_configs.json, -1: small_shapes()), draws, grid_off,
//                                        pilot_off, est_off, res_row
//   pusch_chest_reference_grids.npy      uint32 cbf16 words (re in the low half): per case [P][nof_dmrs][12 nprb], row i what
//                                        receive port i reads (grid port rx_ports[i]), the DM-RS symbols in ascending order, the
//                                        allocated PRBs in ascending order.  The estimator reads nothing else.
//   pusch_chest_reference_pilots.npy     complex64: per case [P][L][6 nprb], the smoothed pilots
//   pusch_chest_reference_estimates.npy  uint32 cbf16 words: per case [L][P][nof_symbols][12 nprb], the estimate on the allocated
//                                        PRBs of symbols first_symbol ...  The recorder marks the estimate beforehand and stops if
//                                        any other element changed, but for this: with a CFO the reference rotates the whole row
//                                        of every symbol of the window, so an unallocated subcarrier's old content comes back
//                                        rotated -- one value of the mark's magnitude per row.  The library leaves those alone.
//   pusch_chest_reference_results.npy    float64 [rows][12], row res_row + port * L + layer: noise variance, RSRP, EPRE, SNR, time
//                                        alignment in seconds (as channel_estimate holds it, a phy_time_unit), CFO in Hz (NaN:
//                                        none), the time alignment the forwarding estimator answered in seconds, that as a bin,
//                                        best and runner-up power in double, the lead asked for, 0
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/dmrs_pusch_estimator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "recorder_grid.h"
// (needs MAX_RB and the generator's interface from the headers above)
#include "lib/phy/upper/signal_processors/dmrs_helper.h"

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
  int              numerology, slot, scrambling_id, n_scid;
  float            scaling;
  std::vector<int> dmrs;
  int              start, ns, layers;
  std::vector<int> ports, prbs;
  int              grid_prb, ue;
  double           snr_db, delay, cfo_hz;
  int              source;
};

// name, numerology, slot, scrambling id, n_scid, beta, DM-RS symbols, first symbol, symbols, layers, rx ports, PRBs, grid PRBs, UE,
// SNR, delay, CFO.
std::vector<Case> small_shapes()
{
  const float      b3 = 1.4125F;
  std::vector<int> ranges = range(3, 6), more = range(15, 25); // range(first, count): PRBs 3-8 and 15-39
  ranges.insert(ranges.end(), more.begin(), more.end());
  ranges.push_back(51);
  std::vector<Case> c = {
      // 5 taps, 6 virtual pilots (the nof_rb == 1 branch), no CFO, no rotation
      {"1 PRB, 1 DM-RS, 1 port", 0, 0, 0, 0, 1.0F, {2}, 0, 14, 1, {0}, {7}, 52, 1, 20, 3, 150, -1},
      // CDM sign on the odd pilots; CFO from the two symbols
      {"1 PRB, 2 DM-RS, 2 layers, ports (1, 0)", 0, 4, 301, 0, b3, {2, 11}, 0, 14, 2, {1, 0}, {5}, 52, 1, 20, 2, -200, -1},
      // 11 taps, 5 virtual pilots
      {"2 PRB, 2 DM-RS", 0, 1, 17, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, {10, 11}, 52, 1, 20, 1, 100, -1},
      // 15 taps, 7 virtual pilots; the third symbol derotated with the measured CFO
      {"3 PRB, 3 DM-RS", 0, 2, 600, 0, 1.0F, {2, 7, 11}, 0, 14, 1, {0}, {20, 21, 22}, 52, 1, 20, -2, 250, -1},
      // the epochs of numerology 1; a window that does not start at symbol 0
      {"4 PRB, 4 DM-RS, mu 1, n_scid 1, window 1..13", 1, 13, 77, 1, 1.0F, {2, 5, 8, 11}, 1, 13, 1, {0}, range(30, 4), 52, 1, 20, 3, -300, -1},
      {"24 PRB, 1 DM-RS at symbol 5, window of 3", 0, 5, 9, 0, 1.0F, {5}, 4, 3, 1, {0}, range(0, 24), 52, 1, 20, 0, 150, -1},
      // 258 pilots: the first count above a stride of 256 threads
      {"43 PRB, 2 layers, 2 ports", 0, 3, 500, 1, b3, {2, 11}, 0, 14, 2, {0, 1}, range(4, 43), 52, 1, 20, 3, 150, -1},
      // more than two strides
      {"86 PRB, 1 layer", 0, 6, 1001, 0, 1.0F, {2, 7, 11}, 0, 14, 1, {0}, range(10, 86), 106, 1, 20, -1, -100, -1},
      // scatter of non-contiguous PRBs; the time alignment sums over the gaps
      {"PRBs 0, 2, 4, 6, 8", 0, 7, 45, 1, 1.0F, {3, 7, 10}, 2, 12, 1, {1}, {0, 2, 4, 6, 8}, 52, 1, 20, 2, 200, -1},
      {"PRBs 3-8, 15-39, 51, ports (3, 1, 0, 2), 2 layers", 0, 8, 123, 0, b3, {2, 5, 8, 11}, 0, 14, 2, {3, 1, 0, 2}, ranges, 52, 1, 20, 1, -150, -1},
      // the kernel's LDS arrays at their limit
      {"273 PRB, 1 port, 1 layer, 2 DM-RS", 0, 9, 1001, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, range(0, 273), 273, 1, 20, 3, 150, -1},
  };
  for (int d : {-40, -3, 3, 40}) { // both halves of the time alignment window
    c.push_back({"25 PRB, delay " + std::to_string(d), 0, 2, 64, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, range(13, 25), 52, 1, 20, (double)d, 100, -1});
  }
  c.push_back({"25 PRB at 0 dB", 0, 3, 64, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, range(13, 25), 52, 1, 0, 2, -100, -1});
  c.push_back({"25 PRB at 40 dB", 0, 4, 64, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, range(13, 25), 52, 1, 40, 2, -100, -1});
  c.push_back({"25 PRB, noise only", 0, 5, 64, 0, 1.0F, {2, 11}, 0, 14, 1, {0}, range(13, 25), 52, 0, 0, 0, 0, -1});
  return c;
}

// pusch_chest_configs.json is written with an indent: its lists hold line breaks.
std::vector<int> json_lines(const std::string& obj, const char* key)
{
  return json_list(obj, key, "0-9, \n");
}

struct PathResult {
  double row[12];
};

struct Reference {
  std::vector<std::vector<cf_t>>             smoothed;
  std::vector<ta_call>                       ta_log;
  std::unique_ptr<dmrs_pusch_estimator_impl> estimator;
  pseudo_random_generator_impl               prg;
  channel_estimate                           estimate;

  Reference()
  {
    dft_processor::configuration dft_cfg;
    dft_cfg.size = DFT;
    dft_cfg.dir  = dft_processor::direction::INVERSE;
    estimator    = std::make_unique<dmrs_pusch_estimator_impl>(
        std::make_unique<pseudo_random_generator_impl>(),
        std::make_unique<port_channel_estimator_average_impl>(
            std::make_unique<interpolator_recorder>(std::make_unique<interpolator_linear_impl>(), smoothed),
            std::make_unique<ta_recorder>(
                std::make_unique<time_alignment_estimator_dft_impl>(std::make_unique<dft_processor_generic_impl>(dft_cfg)), ta_log),
            port_channel_estimator_fd_smoothing_strategy::filter,
            /*compensate_cfo =*/true));
  }

  bounded_bitset<MAX_RB> rb_mask(const Case& c) const
  {
    bounded_bitset<MAX_RB> m(c.grid_prb);
    for (int n : c.prbs) {
      m.set(n);
    }
    return m;
  }

  // The DM-RS of layer 0 on the allocation's pilots (6 per PRB), TS 38.211 Section 6.4.1.1.1, from the reference's generator.
  std::vector<cf_t> dmrs(const Case& c, int symbol)
  {
    const uint64_t n_id = c.scrambling_id;
    const unsigned c_init =
        (unsigned)((((uint64_t)(14 * c.slot + symbol + 1) * (2 * n_id + 1) << 17) + 2 * n_id + c.n_scid) & 0x7FFFFFFFU);
    prg.init(c_init);
    std::vector<cf_t> out(6 * c.prbs.size());
    dmrs_sequence_generate(out, prg, (float)M_SQRT1_2, 0, 6, rb_mask(c));
    return out;
  }

  void run(const word_grid& grid, const Case& c)
  {
    const unsigned                 P = c.ports.size();
    dmrs_pusch_estimator::configuration e;
    e.slot          = slot_point(c.numerology, c.slot);
    e.type          = dmrs_type::TYPE1;
    e.scrambling_id = c.scrambling_id;
    e.n_scid        = c.n_scid != 0;
    e.scaling       = c.scaling;
    e.c_prefix      = cyclic_prefix::NORMAL;
    e.symbols_mask  = bounded_bitset<MAX_NSYMB_PER_SLOT>(14);
    for (int l : c.dmrs) {
      e.symbols_mask.set(l);
    }
    e.rb_mask       = rb_mask(c);
    e.first_symbol  = c.start;
    e.nof_symbols   = c.ns;
    e.nof_tx_layers = c.layers;
    for (unsigned i = 0; i != P; ++i) {
      e.rx_ports.push_back((uint8_t)i);
    }
    // The dimensions estimate() will ask for, so that its resize keeps what is written here.
    estimate.resize({(unsigned)c.grid_prb, (unsigned)(c.start + c.ns), P, (unsigned)c.layers});
    const cbf16_t untouched(7.0F, -7.0F);
    for (unsigned i = 0; i != P; ++i) {
      for (int l = 0; l != c.layers; ++l) {
        span<cbf16_t> path = estimate.get_path_ch_estimate(i, l);
        std::fill(path.begin(), path.end(), untouched);
      }
    }
    smoothed.clear();
    ta_log.clear();
    estimator->estimate(estimate, grid, e);
  }
};

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s pusch_chest_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream     in(argv[1]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  const std::string text = buffer.str();
  const std::string dir  = argv[2];

  std::vector<Case> cases = small_shapes();
  {
    const std::regex object("\\{\\s*\"label\"[^}]*\\}");
    int              index = 0, parity = 0;
    for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it, ++index) {
      const std::string o = it->str();
      if (json_int(o, "dmrs_type") != 1 || o.find("\"ch_estimation\"") == std::string::npos) {
        continue;
      }
      const int        i    = parity++; // its index in parity_cases() of the test file
      std::vector<int> prbs = json_lines(o, "rb_mask");
      if (prbs.size() > 111) {
        continue;
      }
      cases.push_back({"configuration " + std::to_string(index) + ", " + std::to_string(prbs.size()) + " PRB", json_int(o, "numerology"),
                       json_int(o, "slot_index"), json_int(o, "scrambling_id"), json_int(o, "n_scid"), (float)json_float(o, "scaling"),
                       json_lines(o, "dmrs_symbols"), json_int(o, "first_symbol"), json_int(o, "nof_symbols"), json_int(o, "nof_tx_layers"),
                       json_lines(o, "rx_ports"), prbs, json_int(o, "nof_rb"), 1, 15.0 + 5 * (i % 3), (double)(i % 5) - 2.0,
                       100.0 * ((i % 7) - 3), index});
    }
  }

  Reference                              ref;
  std::mt19937                           rng(20241020);
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
    const unsigned            P = c.ports.size(), L = c.layers, nprb = c.prbs.size(), N = 6 * nprb, nd = c.dmrs.size();
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

    std::vector<std::vector<cf_t>> tx(nd); // layer 0's DM-RS per DM-RS symbol
    for (unsigned dd = 0; dd != nd; ++dd) {
      tx[dd] = ref.dmrs(c, c.dmrs[dd]);
    }
    word_grid               grid(P, 12 * c.grid_prb);
    std::vector<PathResult> res(P * L);
    unsigned                draws = 0;
    double                  delay = c.delay;
    bool                    fragile;
    do {
      ++draws;
      delay = c.delay + (c.ue ? uniform(rng) - 0.5 : 0.0);
      const double sigma = std::sqrt(std::pow(10.0, -c.snr_db / 10.0) / 2); // per component
      for (unsigned p = 0; p != P; ++p) {
        std::vector<cd> acc(nd * 12 * nprb, 0.0);
        for (unsigned l = 0; l != L && c.ue; ++l) {
          const cd g0 = std::polar(1.0, 2 * M_PI * uniform(rng)), g1 = std::polar(0.5, 2 * M_PI * uniform(rng));
          for (unsigned dd = 0; dd != nd; ++dd) {
            for (unsigned q = 0; q != N; ++q) {
              const double k = subc[2 * q];
              const cd     h = g0 * std::polar(1.0, -2 * M_PI * k * delay / DFT) + g1 * std::polar(1.0, -2 * M_PI * k * (delay + 4) / DFT);
              const double w = (l == 1 && (q & 1)) ? -1.0 : 1.0; // port 1001: w_f = (+1, -1)
              acc[dd * 12 * nprb + 2 * q] += h * ((double)c.scaling * w) * cd(tx[dd][q].real(), tx[dd][q].imag());
            }
          }
        }
        for (unsigned dd = 0; dd != nd; ++dd) {
          const cd rot = std::polar(1.0, 2 * M_PI * (c.cfo_hz / scs) * ep[c.dmrs[dd]]);
          for (unsigned j = 0; j != 12 * nprb; ++j) {
            const cd v = acc[dd * 12 * nprb + j] * rot + sigma * cd(normal(rng), normal(rng));
            grid.set(p, c.dmrs[dd], subc[j], (float)v.real(), (float)v.imag());
          }
        }
      }
      ref.run(grid, c);
      if (ref.smoothed.size() != P * L || ref.ta_log.size() != P * L) {
        std::fprintf(stderr, "case %zu: %zu interpolations and %zu time alignments for %u paths\n", ic, ref.smoothed.size(), ref.ta_log.size(), P * L);
        return 1;
      }
      fragile = false;
      for (unsigned p = 0; p != P; ++p) {
        for (unsigned l = 0; l != L; ++l) {
          const std::vector<cf_t>& f  = ref.smoothed[p * L + l];
          const ta_call&           ta = ref.ta_log[p * L + l];
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
          fragile             = fragile || (best - second < asked * best);
          const double   bin  = ta.answer * DFT * scs;
          const unsigned path = p * L + l;
          const double   row[12] = {ref.estimate.get_noise_variance(p, l), ref.estimate.get_rsrp(p, l), ref.estimate.get_epre(p, l),
                                    ref.estimate.get_snr(p, l), ref.estimate.get_time_alignment(p, l).to_seconds(),
                                    ref.estimate.get_cfo_Hz(p, l).has_value() ? (double)ref.estimate.get_cfo_Hz(p, l).value() : NaN,
                                    ta.answer, std::round(bin), best, second, asked, 0.0};
          std::memcpy(res[path].row, row, sizeof(row));
          if (!fragile && (std::fabs(bin - std::round(bin)) > 1e-6 || (int)std::round(bin) != best_bin)) {
            std::fprintf(stderr, "case %zu port %u layer %u: the reference's bin %g, %d in double with a lead of %g\n", ic, p, l, bin, best_bin,
                         (best - second) / best);
            return 1;
          }
        }
      }
    } while (fragile && draws != 10000);
    if (fragile) {
      std::fprintf(stderr, "case %zu (%s): every draw fragile\n", ic, c.name.c_str());
      return 1;
    }
    draws_total += draws;

    const size_t grid_off = grids.size(), pilot_off = pilots.size(), est_off = estimates.size(), res_row = results.size() / 12;
    for (unsigned p = 0; p != P; ++p) {
      for (int l : c.dmrs) {
        for (unsigned k : subc) {
          grids.push_back(grid.word(p, l, k));
        }
      }
      for (unsigned l = 0; l != L; ++l) {
        pilots.insert(pilots.end(), ref.smoothed[p * L + l].begin(), ref.smoothed[p * L + l].end());
        results.insert(results.end(), res[p * L + l].row, res[p * L + l].row + 12);
      }
    }
    // The estimate: the region in [L][P][symbol][allocated subcarrier] order, nothing else written.
    const uint32_t    same = word_of(cbf16_t(7.0F, -7.0F));
    std::vector<bool> allocated(12 * c.grid_prb, false);
    for (unsigned k : subc) {
      allocated[k] = true;
    }
    for (unsigned l = 0; l != L; ++l) {
      for (unsigned p = 0; p != P; ++p) {
        for (int s = 0; s != c.start + c.ns; ++s) {
          span<const cbf16_t> row = ref.estimate.get_symbol_ch_estimate(s, p, l);
          // With a CFO the reference rotates the whole row of every symbol of the window, the unallocated subcarriers' old
          // content included: there the mark may come back as one rotated value of its magnitude, and as nothing else.
          uint32_t mark = same;
          for (unsigned k = 0; k != row.size(); ++k) {
            if (!allocated[k]) {
              mark = word_of(row[k]);
              break;
            }
          }
          const cf_t   m      = cf_t(bf16_value(mark & 0xFFFFU), bf16_value(mark >> 16));
          const bool   rotate = s >= c.start && nd >= 2;
          if (mark != same && !(rotate && std::fabs(std::abs(m) - std::sqrt(98.0F)) < 0.05F)) {
            std::fprintf(stderr, "case %zu: layer %u port %u symbol %d was written outside the allocation\n", ic, l, p, s);
            return 1;
          }
          for (unsigned k = 0; k != row.size(); ++k) {
            const bool inside = s >= c.start && allocated[k];
            if (inside) {
              estimates.push_back(word_of(row[k]));
            } else if (word_of(row[k]) != mark) {
              std::fprintf(stderr, "case %zu: layer %u port %u symbol %d subcarrier %u was written\n", ic, l, p, s, k);
              return 1;
            }
          }
        }
      }
    }
    char num[128];
    std::snprintf(num, sizeof(num), "\"scaling\": %.9g, \"snr_db\": %.17g, \"delay\": %.17g, \"cfo_hz\": %.17g", (double)c.scaling, c.snr_db, delay, c.cfo_hz);
    json << (ic ? ",\n" : "") << "{\"name\": \"" << c.name << "\", \"numerology\": " << c.numerology << ", \"slot_index\": " << c.slot
         << ", \"scrambling_id\": " << c.scrambling_id << ", \"n_scid\": " << c.n_scid << ", " << num << ", \"dmrs_symbols\": " << list_json(c.dmrs)
         << ", \"first_symbol\": " << c.start << ", \"nof_symbols\": " << c.ns << ", \"nof_tx_layers\": " << c.layers
         << ", \"rx_ports\": " << list_json(c.ports) << ", \"prbs\": " << list_json(c.prbs) << ", \"grid_prb\": " << c.grid_prb << ", \"ue\": " << c.ue
         << ", \"source\": " << c.source << ", \"draws\": " << draws << ", \"grid_off\": " << grid_off << ", \"pilot_off\": " << pilot_off
         << ", \"est_off\": " << est_off << ", \"res_row\": " << res_row << "}";
    std::printf("case %2zu: %u draws, lead asked %.3g  %s\n", ic, draws, asked, c.name.c_str());
  }
  json << "\n]\n";
  std::ofstream(dir + "/pusch_chest_reference_cases.json") << json.str();
  write_npy(dir + "/pusch_chest_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pusch_chest_reference_pilots.npy", "<c8", pilots, 0);
  write_npy(dir + "/pusch_chest_reference_estimates.npy", "<u4", estimates, 0);
  write_npy(dir + "/pusch_chest_reference_results.npy", "<f8", results, 12);
  std::printf("%zu cases, %zu draws; %zu grid words, %zu pilots, %zu estimate words, %zu result rows\n", cases.size(), draws_total, grids.size(),
              pilots.size(), estimates.size(), results.size() / 12);
  return 0;
}
