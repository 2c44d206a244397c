// Records the answers of srsRAN-5G-ER's prach_detector_generic_impl (combine_symbols = true) and prach_generator_impl for
// tests/test_prach_detector.py.  It constructs the reference's classes directly -- the detector over two
// dft_processor_generic_impl (1024 and 256 points, inverse) and a prach_generator_impl, on a prach_buffer_impl --, makes an
// occasion per case with a transmitter of its own, and writes inputs and outputs as .npy files.  Built and run by
// oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`,
// `make -C oracle rerecord-check`; no binary or object is committed.
//
// Cases: the entries of prach_detector_configs.json that the reference's validator accepts (48 of 60; the others are red rows
// of its threshold table), each carrying its preamble_index delayed by true_delay, its root sequence index reduced modulo
// L - 1; then the edge shapes of EDGES below.  Only rows of the threshold table that are not red are used: formats 0, 1, A1,
// A2 and B4, which give 1, 2, 4 and 12 symbols (every row of format 2 is red, and formats 3, A3, B1, C0 and C2 have no row).
//
// The transmitter.  Element k of every symbol of port p is
//   sum over the preambles t of a_t y_t[k] / sqrt(L) exp(-j 2 pi k d_t / N) exp(j phi_tp)  +  noise,
// y_t the reference generator's sequence, d_t a delay in correlation samples, phi_tp a random phase and the noise complex Gaussian
// of unit variance (of standard deviation `level` where a case states one), independent per element.  Every component is rounded to a multiple of 2^-e, e the largest exponent at which
// the case fits int16; the int16 pairs are stored and the detector is fed exactly those values widened to float.  The amplitude
// a_t is found by iteration so that the preamble's window peaks at `target` times the threshold (1.5 ... 20), or at 0.7 of what
// it reaches far above the noise where that is less: the leakage of a fractional delay out of the reference window bounds it.
//
// The IDFT is handed to the detector inside a forwarding dft_processor that keeps every run() output.  From those outputs the
// recorder evaluates each monitored window in double, for one purpose: an occasion in which a monitored window's peak lies
// within 2 % of the threshold, or in which a window whose peak exceeds the threshold has its two largest samples within 2 % of
// the larger, is drawn again.  No recorded decision is fragile, so a test sets nothing aside.
//
// Files (case i is row i of `cases` and of `results`):
//   prach_detector_reference_cases.npy      int32 [n][16]: format (0, 1, 2, 3, A1, A2, A3, B1, B4, C0, C2 as 0..10), ra_scs (15,
//                                           30, 60, 120, 1.25, 5 kHz as 0..5), root_sequence_index, zero_correlation_zone,
//                                           start_preamble_index, nof_preamble_indices, nof_rx_ports, e (an input value is its
//                                           int16 times 2^-e), input file k, offset into it in pairs, pairs
//                                           (ports x symbols x L), first row in `detections`, number of detections, group (0: an
//                                           entry of prach_detector_configs.json, 1: an edge shape), index of the entry or of the
//                                           edge shape, number of preambles transmitted
//   prach_detector_reference_in<k>.npy      int16 [..][2]: (re, im), the occasions back to back, each as [port][symbol][L]; a
//                                           file holds whole cases and stays below 900000 bytes
//   prach_detector_reference_results.npy    float64 [n][3]: rssi_dB, time_resolution and time_advance_max in seconds
//   prach_detector_reference_detections.npy float64 [m][3]: preamble index, time advance in seconds, detection_metric, in the
//                                           order the reference reported them
//   prach_detector_reference_sequences.npy  float32 pairs: per tuple of SEQUENCES the pairs (format, root_sequence_index),
//                                           (zero_correlation_zone, preamble_index) and then the L values of
//                                           prach_generator_impl::generate
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/prach_buffer_impl.h"
#include "lib/phy/upper/channel_processors/prach_detector_generic_impl.h"
#include "lib/phy/upper/channel_processors/prach_detector_generic_thresholds.h"
#include "lib/phy/upper/channel_processors/prach_generator_impl.h"
#include "recorder_io.h"
#include "srsran/ran/prach/prach_cyclic_shifts.h"
#include "srsran/ran/prach/prach_preamble_information.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <random>

using namespace srsran;

namespace {

const char* FORMATS[11] = {"0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2"};
const char* SPACINGS[6] = {"15", "30", "60", "120", "1.25", "5"};
enum { F0 = 0, F1 = 1, A1 = 4, A2 = 5, B4 = 8 };
enum { K15 = 0, K30 = 1, K1_25 = 4 };
enum { NORMAL, ZERO, TINY };

struct Tx {
  int    preamble;
  double delay;  // in correlation samples
  double target; // > 0: the window's peak over the threshold to aim at; < 0: the amplitude -target as it is
};

struct Case {
  int              format, scs, root, zcz, start, nof, ports;
  std::vector<Tx>  tx;
  int              kind;
  std::vector<int> expect;        // the preambles the reference must report
  double           level = 1.0;   // the standard deviation of the noise; the amplitudes scale with it
  int              dead_ports = 0; // so many of the last ports are all zero
};

// The edge shapes.  {format, spacing, root, zcz, start, nof, ports}, {preamble, delay, target}..., kind, expected report.
const std::vector<Case> EDGES = {
    // Window 0, whose reference window starts below zero and wraps, and window 63, the last of the root (N_CS 13: one root).
    {F0, K1_25, 77, 1, 0, 64, 2, {{0, 3, 4}, {63, 5, 6}}, NORMAL, {0, 63}},
    // Two preambles in adjacent windows of one root.
    {F0, K1_25, 5, 1, 0, 64, 2, {{20, 3, 2.5}, {21, 5, 5}}, NORMAL, {20, 21}},
    // max_delay 14: 11 is the last delay below 0.8 x 14 = 11.2 ...
    {F0, K1_25, 100, 1, 0, 64, 1, {{0, 11, 10}}, NORMAL, {0}},
    // ... and 12 the first beyond it: the peak is above the threshold, inside the window (15 samples), and not reported.
    {F0, K1_25, 100, 1, 0, 64, 1, {{0, 12, 10}}, NORMAL, {}},
    // max_delay 40: float(40) x 0.8 is 32 in double, so 31 is reported ...
    {A2, K15, 30, 11, 0, 64, 2, {{0, 31, 10}}, NORMAL, {0}},
    // ... and 32, equal to the bound, is not (0.8f widened to double would make the bound 32.0000005 and report it).
    {A2, K15, 30, 11, 0, 64, 2, {{0, 32, 10}}, NORMAL, {}},
    // N_CS 32: 26 shifts per root, so the third root is used for 12 preambles only.  The last window of the first root, window 0
    // of the second, a preamble of the third; 4 ports.
    {F0, K1_25, 400, 6, 0, 64, 4, {{25, 4, 3}, {26, 2, 5}, {60, 10, 12}}, NORMAL, {25, 26, 60}},
    // A root index two below the table's end: the third root wraps to index 0.
    {F0, K1_25, 836, 6, 0, 64, 1, {{30, 7, 4}, {55, 5, 7}}, NORMAL, {30, 55}},
    // zcz 0: one shift per root, 64 roots, win_width = cp_prach (875 of 1024 samples in format 1); the roots wrap from 837 to 0.
    {F1, K1_25, 830, 0, 0, 64, 1, {{3, 20, 5}, {12, 400, 8}}, NORMAL, {3, 12}},
    // zcz 0 on a short format at 30 kHz with 4 ports; the roots wrap from 137 to 0.
    {A1, K30, 136, 0, 0, 64, 4, {{5, 10, 3}, {40, 20, 9}}, NORMAL, {5, 40}},
    // N_CS 46 on 139: 3 shifts per root, 22 roots, the last holds preamble 63 alone; the roots wrap; 12 symbols.
    {B4, K30, 120, 14, 0, 64, 2, {{2, 50, 4}, {3, 1, 6}, {63, 30, 15}}, NORMAL, {2, 3, 63}},
    // A monitored range [20, 60) that starts and ends inside a root's shifts (46 per root); its first and its last preamble, and
    // one just outside at either end, which are not reported.
    {F0, K1_25, 300, 3, 20, 40, 2, {{19, 3, 10}, {20, 3, 4}, {59, 6, 5}, {60, 4, 10}}, NORMAL, {20, 59}},
    // A monitored range of one preamble, its neighbour transmitted too.
    {A1, K15, 50, 7, 37, 1, 1, {{37, 4, 6}, {38, 4, 10}}, NORMAL, {37}},
    // zcz 0 with a part of the roots monitored; preamble 9 belongs to a root that is not correlated at all.
    {A2, K15, 50, 0, 10, 20, 1, {{9, 3, -1.0}, {15, 30, 5}}, NORMAL, {15}},
    // Six preambles over five roots (N_CS 59: 14 shifts per root): many windows report, and the roots interfere.
    {F0, K1_25, 200, 9, 0, 64, 2, {{1, 10, 3}, {13, 40, 5}, {14, 2, 8}, {30, 25, 2}, {45, 50, 12}, {63, 7, 20}}, NORMAL,
     {1, 13, 14, 30, 45, 63}},
    // Four preambles over four roots of a short format at 30 kHz (N_CS 15: 9 shifts per root), 4 ports, 4 symbols.  On 139
    // elements the other roots' preambles are a floor of 1 / 139 each, which bounds the number and the targets.
    {A2, K30, 10, 8, 0, 64, 4, {{8, 12, 2}, {9, 1, 3}, {33, 15, 3}, {63, 10, 4}}, NORMAL, {8, 9, 33, 63}},
    // Adjacent windows on 12 symbols at 15 kHz with 4 ports.
    {B4, K15, 60, 11, 0, 64, 4, {{13, 7, 3}, {14, 9, 6}}, NORMAL, {13, 14}},
    // A receive port that is all zero at a low level (2^-14): its reference - value is 0, not normal, so the port adds the
    // reference's 1e-9 to the denominator, where the live ports add about 2.5e-9.  The metric is a ratio, so this is the only
    // place where the scale of the combined symbols shows (a sum over the symbols, not a mean).
    {A2, K15, 90, 5, 0, 64, 2, {{7, 4, 5}}, NORMAL, {7}, 6.103515625e-05, 1},
    {B4, K30, 20, 9, 0, 64, 4, {{20, 6, 4}, {43, 11, 8}}, NORMAL, {20, 43}, 6.103515625e-05, 2},
    // Noise only.
    {F0, K1_25, 9, 1, 0, 64, 1, {}, NORMAL, {}},
    {B4, K15, 70, 5, 0, 64, 4, {}, NORMAL, {}},
    {A1, K30, 3, 4, 0, 64, 2, {}, NORMAL, {}},
    // All zero: the early return, rssi_dB = -inf.
    {F0, K1_25, 5, 1, 0, 64, 2, {}, ZERO, {}},
    {B4, K15, 5, 11, 0, 64, 1, {}, ZERO, {}},
    // A strong preamble at an amplitude at which the RSSI is subnormal in float32: the early return, with a finite rssi_dB.
    {F0, K1_25, 40, 1, 0, 64, 1, {{7, 4, 10}}, TINY, {}},
    {A2, K15, 40, 5, 0, 64, 2, {{7, 4, 10}}, TINY, {}},
};

// The generator's tuples: {format, root_sequence_index, zcz, preamble}.
const int SEQUENCES[][4] = {
    {F0, 0, 0, 0},     // the first root
    {F0, 837, 0, 0},   // the last root, L - 2
    {F0, 837, 1, 63},  // its last shift
    {F0, 400, 15, 63}, // N_CS 419: two shifts per root, root 431, shift 419
    {F0, 836, 0, 10},  // the root index wraps to 8
    {F1, 123, 15, 1},  // format 1 takes format 0's N_CS table
    {B4, 0, 0, 0},     // short: the first root
    {B4, 137, 0, 0},   // the last root, L - 2
    {A1, 137, 15, 63}, // N_CS 69: root 137 + 31 wraps to 30, shift 69
    {A2, 50, 5, 17},   // N_CS 10
    {B4, 136, 0, 63},  // wraps to 61
    {A1, 22, 7, 40},   // N_CS 13
};

// Forwards to the reference's transform and keeps every output.
class idft_recorder : public dft_processor
{
  std::unique_ptr<dft_processor>  inner;
  std::vector<std::vector<cf_t>>& log;

public:
  idft_recorder(std::unique_ptr<dft_processor> inner_, std::vector<std::vector<cf_t>>& log_) : inner(std::move(inner_)), log(log_) {}
  direction        get_direction() const override { return inner->get_direction(); }
  unsigned         get_size() const override { return inner->get_size(); }
  span<cf_t>       get_input() override { return inner->get_input(); }
  span<const cf_t> run() override
  {
    span<const cf_t> out = inner->run();
    log.emplace_back(out.begin(), out.end());
    return out;
  }
};

// What the recorder needs to find the windows in the logged outputs.
struct Shape {
  unsigned L, N, nsym, n_cs, shifts, sequences, win, margin;
  double   threshold;
};

Shape shape_of(const prach_detector::configuration& c)
{
  static const detail::threshold_and_margin_finder finder(detail::all_threshold_and_margins);
  const prach_preamble_information info = is_long_preamble(c.format) ? get_prach_preamble_long_info(c.format)
                                                                     : get_prach_preamble_short_info(c.format, c.ra_scs, false);
  Shape s;
  s.L         = info.sequence_length;
  s.N         = s.L == 839 ? 1024 : 256;
  s.nsym      = info.nof_symbols;
  s.n_cs      = prach_cyclic_shifts_get(c.ra_scs, c.restricted_set, c.zero_correlation_zone);
  s.shifts    = s.n_cs == 0 ? 1 : std::min(64U, s.L / s.n_cs);
  s.sequences = (64 + s.shifts - 1) / s.shifts;
  const unsigned cp = (unsigned)std::floor(info.cp_length.to_seconds() * s.L * ra_scs_to_Hz(info.scs));
  s.win             = ((s.n_cs == 0 ? cp : std::min(s.n_cs, cp)) * s.N) / s.L;
  detail::threshold_params p;
  p.nof_rx_ports          = c.nof_rx_ports;
  p.scs                   = c.ra_scs;
  p.format                = c.format;
  p.zero_correlation_zone = c.zero_correlation_zone;
  p.combine_symbols       = true;
  const auto th = finder.get(p);
  s.threshold   = th.first;
  s.margin      = th.second;
  return s;
}

struct Window {
  double top[2]; // the two largest samples of the metric
};

// The metric of every window of every correlated root, in double, from the logged transform outputs ([root][port]).
std::vector<Window> evaluate(const std::vector<std::vector<cf_t>>& log, const Shape& s, unsigned ports, const std::vector<unsigned>& roots)
{
  std::vector<Window> out(64, Window{{-1.0, -1.0}});
  for (size_t r = 0; r != roots.size(); ++r) {
    for (unsigned w = 0; w != s.shifts; ++w) {
      const unsigned      start = (s.N - (s.n_cs * w * s.N) / s.L) % s.N;
      std::vector<double> num(s.win, 0.0), den(s.win, 0.0);
      for (unsigned p = 0; p != ports; ++p) {
        const std::vector<cf_t>& c = log[r * ports + p];
        auto                     m = [&](unsigned i) { return (double)std::norm(std::complex<double>(c[i].real(), c[i].imag())) / ((double)s.N * s.L * s.L); };
        double                   reference = 0.0;
        for (unsigned j = 0; j != 2 * s.margin + s.win; ++j) {
          reference += m((start + s.N - s.margin + j) % s.N);
        }
        for (unsigned i = 0; i != s.win; ++i) {
          const double v    = m(start + i) * (double)s.N / (double)s.L;
          const double diff = reference - v;
          num[i] += v;
          den[i] += std::isnormal(diff) ? diff : 1e-9;
        }
      }
      const unsigned preamble = roots[r] * s.shifts + w;
      if (preamble >= 64) {
        continue;
      }
      for (unsigned i = 0; i != s.win; ++i) {
        const double v = num[i] / std::abs(den[i]);
        if (v > out[preamble].top[0]) {
          out[preamble].top[1] = out[preamble].top[0];
          out[preamble].top[0] = v;
        } else if (v > out[preamble].top[1]) {
          out[preamble].top[1] = v;
        }
      }
    }
  }
  return out;
}

template <typename T>
int index_of(T& names, const std::string& name)
{
  for (int i = 0; i != (int)std::size(names); ++i) {
    if (name == names[i]) {
      return i;
    }
  }
  std::fprintf(stderr, "unknown name %s\n", name.c_str());
  std::exit(1);
}

prach_detector::configuration to_config(const Case& c)
{
  prach_detector::configuration cfg;
  cfg.root_sequence_index   = c.root;
  cfg.format                = to_prach_format_type(FORMATS[c.format]);
  cfg.restricted_set        = restricted_set_config::UNRESTRICTED;
  cfg.zero_correlation_zone = c.zcz;
  cfg.start_preamble_index  = c.start;
  cfg.nof_preamble_indices  = c.nof;
  cfg.ra_scs                = static_cast<prach_subcarrier_spacing>(c.scs);
  cfg.nof_rx_ports          = c.ports;
  return cfg;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s prach_detector_configs.json OUT\n", argv[0]);
    return 2;
  }
  std::ifstream     in(argv[1]);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string text = ss.str();
  const std::string dir  = argv[2];

  std::vector<std::vector<cf_t>> log;
  auto idft = [&log](unsigned size) {
    return std::make_unique<idft_recorder>(
        std::make_unique<dft_processor_generic_impl>(dft_processor::configuration{size, dft_processor::direction::INVERSE}), log);
  };
  prach_detector_generic_impl   detector(idft(1024), idft(256), std::make_unique<prach_generator_impl>(), true);
  prach_detector_validator_impl validator;
  prach_generator_impl          generator;

  // The cases: the accepted entries of the fixture, then the edge shapes.
  std::vector<Case> cases;
  std::vector<int>  group, origin;
  const std::regex  object("\\{\"root_sequence_index\"[^}]*\\}");
  static const double TARGETS[4] = {1.5, 3.0, 8.0, 20.0};
  int                 entry      = 0;
  for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it, ++entry) {
    const std::string o = it->str();
    Case              c = {index_of(FORMATS, json_field(o, "format")), index_of(SPACINGS, json_field(o, "ra_scs")), 0,
                           std::stoi(json_field(o, "zero_correlation_zone")), std::stoi(json_field(o, "start_preamble_index")),
                           std::stoi(json_field(o, "nof_preamble_indices")), std::stoi(json_field(o, "nof_rx_ports")), {}, NORMAL, {}};
    const int         L = c.format < 4 ? 839 : 139, N = c.format < 4 ? 1024 : 256;
    c.root              = std::stoi(json_field(o, "root_sequence_index")) % (L - 1);
    if (!validator.is_valid(to_config(c))) {
      continue;
    }
    const int    preamble = std::stoi(json_field(o, "preamble_index"));
    const double delay    = std::stod(json_field(o, "true_delay")) * N * ra_scs_to_Hz(static_cast<prach_subcarrier_spacing>(c.scs));
    c.tx.push_back({preamble, delay, TARGETS[cases.size() % 4]});
    c.expect.push_back(preamble);
    cases.push_back(c);
    group.push_back(0);
    origin.push_back(entry);
  }
  const size_t nof_reference = cases.size();
  for (size_t i = 0; i != EDGES.size(); ++i) {
    if (!validator.is_valid(to_config(EDGES[i]))) {
      std::fprintf(stderr, "edge shape %zu is a red row\n", i);
      return 1;
    }
    cases.push_back(EDGES[i]);
    group.push_back(1);
    origin.push_back((int)i);
  }

  std::mt19937_64                        rng(20241019);
  std::normal_distribution<double>       normal(0.0, 1.0);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  std::vector<int32_t>                   rows;
  std::vector<double>                    results, detections;
  std::vector<int16_t>                   shard;
  int                                    shard_index = 0;
  auto flush = [&]() {
    write_npy(dir + "/prach_detector_reference_in" + std::to_string(shard_index) + ".npy", "<i2", shard, 2);
    shard.clear();
    ++shard_index;
  };
  double lowest = 1e9, highest = 0.0;
  for (size_t ic = 0; ic != cases.size(); ++ic) {
    const Case&                         c   = cases[ic];
    const prach_detector::configuration cfg = to_config(c);
    const Shape                         s   = shape_of(cfg);
    const size_t                        n   = (size_t)c.ports * s.nsym * s.L;
    std::vector<unsigned>               roots;
    for (unsigned q = 0; q != s.sequences; ++q) {
      if (q * s.shifts < (unsigned)(c.start + c.nof) && (q + 1) * s.shifts > (unsigned)c.start) {
        roots.push_back(q);
      }
    }
    auto window_is_evaluated = [&](int preamble) { return std::find(roots.begin(), roots.end(), (unsigned)preamble / s.shifts) != roots.end(); };
    // The sequences of the transmitted preambles, at unit amplitude with their delays.
    std::vector<std::vector<std::complex<double>>> waves;
    for (const Tx& t : c.tx) {
      prach_generator::configuration g;
      g.format                = cfg.format;
      g.root_sequence_index   = c.root;
      g.preamble_index        = t.preamble;
      g.restricted_set        = cfg.restricted_set;
      g.zero_correlation_zone = c.zcz;
      span<const cf_t>                  y = generator.generate(g);
      std::vector<std::complex<double>> wave(s.L);
      for (unsigned k = 0; k != s.L; ++k) {
        wave[k] = std::complex<double>(y[k].real(), y[k].imag()) / std::sqrt((double)s.L) *
                  std::polar(1.0, -2.0 * M_PI * (double)k * t.delay / (double)s.N);
      }
      waves.push_back(wave);
      if (t.target > 0 && !window_is_evaluated(t.preamble)) {
        std::fprintf(stderr, "case %zu: preamble %d has a target but its root is not correlated\n", ic, t.preamble);
        return 1;
      }
    }

    prach_buffer_impl                 buffer(c.ports, 1, 1, s.nsym, s.L);
    std::vector<int16_t>              words(2 * n, 0);
    int                               e = 0;
    prach_detection_result            result;
    std::vector<std::complex<double>> noise(n), clean(n);
    std::vector<double>               amplitude(c.tx.size());
    auto run = [&]() {
      for (unsigned p = 0; p != (unsigned)c.ports; ++p) {
        for (unsigned l = 0; l != s.nsym; ++l) {
          span<cf_t> symbol = buffer.get_symbol(p, 0, 0, l);
          for (unsigned k = 0; k != s.L; ++k) {
            const size_t i = ((size_t)p * s.nsym + l) * s.L + k;
            symbol[k]      = cf_t(std::ldexp((float)words[2 * i], -e), std::ldexp((float)words[2 * i + 1], -e));
          }
        }
      }
      log.clear();
      result = detector.detect(buffer, cfg);
    };
    bool     good     = c.kind == ZERO;
    unsigned attempts = 0;
    while (!good && attempts++ != 1000) {
      std::vector<double> phase(c.tx.size() * c.ports);
      for (double& v : phase) {
        v = 2.0 * M_PI * uniform(rng);
      }
      for (std::complex<double>& v : noise) {
        v = std::complex<double>(normal(rng), normal(rng)) * std::sqrt(0.5);
      }
      for (size_t t = 0; t != c.tx.size(); ++t) {
        amplitude[t] = (c.tx[t].target > 0 ? 0.2 : -c.tx[t].target) * c.level;
      }
      std::vector<Window> windows;
      std::vector<double> target(c.tx.size());
      bool                converged = false;
      for (unsigned iteration = 0; iteration != 40 + c.tx.size() && !converged; ++iteration) {
        // The first runs carry one preamble each, far above the noise: what the leakage out of the reference window lets its
        // metric reach.
        const bool          alone = iteration < c.tx.size();
        std::vector<double> a     = amplitude;
        if (alone) {
          std::fill(a.begin(), a.end(), 0.0);
          a[iteration] = 1000.0 * c.level;
        }
        double largest = 0.0;
        for (size_t i = 0; i != n; ++i) {
          const unsigned p = i / (s.nsym * s.L), k = i % s.L;
          clean[i] = c.level * noise[i];
          for (size_t t = 0; t != c.tx.size(); ++t) {
            clean[i] += a[t] * waves[t][k] * std::polar(1.0, phase[t * c.ports + p]);
          }
          if (p + c.dead_ports >= (unsigned)c.ports) {
            clean[i] = 0.0;
          }
          largest = std::max({largest, std::abs(clean[i].real()), std::abs(clean[i].imag())});
        }
        e = (int)std::floor(std::log2(32767.0 / largest));
        for (size_t i = 0; i != n; ++i) {
          words[2 * i]     = (int16_t)std::lrint(std::ldexp(clean[i].real(), e));
          words[2 * i + 1] = (int16_t)std::lrint(std::ldexp(clean[i].imag(), e));
        }
        run();
        if (log.size() != roots.size() * c.ports) {
          std::fprintf(stderr, "case %zu: %zu transforms\n", ic, log.size());
          return 1;
        }
        windows = evaluate(log, s, c.ports, roots);
        if (alone) {
          const size_t t = iteration;
          if (c.tx[t].target > 0) {
            target[t] = std::min(c.tx[t].target, 0.7 * windows[c.tx[t].preamble].top[0] / s.threshold);
            if (target[t] < 1.15) {
              std::fprintf(stderr, "case %zu: preamble %d reaches %.2f of the threshold at most\n", ic, c.tx[t].preamble, target[t] / 0.7);
              return 1;
            }
          }
          continue;
        }
        converged = true;
        for (size_t t = 0; t != c.tx.size(); ++t) {
          if (c.tx[t].target > 0) {
            const double ratio = windows[c.tx[t].preamble].top[0] / s.threshold / target[t];
            if (std::abs(ratio - 1.0) > 0.1) {
              converged = false;
              amplitude[t] *= std::min(1.5, std::max(0.5, std::sqrt(1.0 / ratio)));
            }
          }
        }
      }
      if (!converged) {
        continue;
      }
      good = true;
      for (int i = c.start; i != c.start + c.nof; ++i) { // the two conditions
        const double* top = windows[i].top;
        if (std::abs(top[0] / s.threshold - 1.0) < 0.02 || (top[0] > s.threshold && top[0] - top[1] <= 0.02 * top[0])) {
          good = false;
        }
      }
      std::vector<int> reported;
      for (const auto& p : result.preambles) {
        reported.push_back(p.preamble_index);
        if (p.detection_metric < 1.05 || p.detection_metric > 50.0) {
          good = false;
        }
      }
      std::vector<int> expect = c.kind == TINY ? std::vector<int>{c.tx[0].preamble} : c.expect;
      if (good && reported != expect) {
        std::fprintf(stderr, "case %zu, attempt %u: reported", ic, attempts);
        for (int v : reported) {
          std::fprintf(stderr, " %d", v);
        }
        std::fprintf(stderr, "\n");
        good = false;
      }
    }
    if (!good) {
      std::fprintf(stderr, "case %zu: no occasion met the conditions\n", ic);
      return 1;
    }
    if (c.kind == TINY) { // the same int16 values at a smaller scale, until the RSSI is subnormal
      const float rssi = std::pow(10.0F, result.rssi_dB / 10.0F);
      e += (int)std::ceil(0.5 * std::log2((double)rssi / (0.5 * 1.17549435e-38)));
      run();
      const float tiny = std::pow(10.0F, result.rssi_dB / 10.0F);
      if (!result.preambles.empty() || !std::isfinite(result.rssi_dB) || std::isnormal(tiny) || !log.empty()) {
        std::fprintf(stderr, "case %zu: not the early return (rssi_dB %g)\n", ic, result.rssi_dB);
        return 1;
      }
    } else if (c.kind == ZERO) {
      run();
      if (!result.preambles.empty() || !log.empty()) {
        std::fprintf(stderr, "case %zu: not the early return\n", ic);
        return 1;
      }
    }
    if ((shard.size() + 2 * n) * sizeof(int16_t) > 900000 - 128) {
      flush();
    }
    const int32_t row[16] = {c.format, c.scs, c.root, c.zcz, c.start, c.nof, c.ports, e, shard_index, (int32_t)(shard.size() / 2), (int32_t)n,
                             (int32_t)(detections.size() / 3), (int32_t)result.preambles.size(), group[ic], origin[ic], (int32_t)c.tx.size()};
    rows.insert(rows.end(), row, row + 16);
    shard.insert(shard.end(), words.begin(), words.end());
    results.push_back(result.rssi_dB);
    results.push_back(result.time_resolution.to_seconds());
    results.push_back(result.time_advance_max.to_seconds());
    for (const auto& p : result.preambles) {
      detections.push_back(p.preamble_index);
      detections.push_back(p.time_advance.to_seconds());
      detections.push_back(p.detection_metric);
      lowest  = std::min(lowest, (double)p.detection_metric);
      highest = std::max(highest, (double)p.detection_metric);
    }
    std::printf("case %zu: %u attempt(s), %zu reported, rssi %.3f dB\n", ic, attempts, result.preambles.size(), result.rssi_dB);
  }
  flush();
  write_npy(dir + "/prach_detector_reference_cases.npy", "<i4", rows, 16);
  write_npy(dir + "/prach_detector_reference_results.npy", "<f8", results, 3);
  write_npy(dir + "/prach_detector_reference_detections.npy", "<f8", detections, 3);

  std::vector<float> sequences;
  for (const auto& q : SEQUENCES) {
    prach_generator::configuration g;
    g.format                = to_prach_format_type(FORMATS[q[0]]);
    g.root_sequence_index   = q[1];
    g.preamble_index        = q[3];
    g.restricted_set        = restricted_set_config::UNRESTRICTED;
    g.zero_correlation_zone = q[2];
    for (int v : q) {
      sequences.push_back((float)v);
    }
    for (const cf_t& v : generator.generate(g)) {
      sequences.push_back(v.real());
      sequences.push_back(v.imag());
    }
  }
  write_npy(dir + "/prach_detector_reference_sequences.npy", "<f4", sequences, 2);
  std::printf("%zu cases (%zu of the reference's) in %d input files, %zu detections with metrics %.2f ... %.2f, %zu sequences\n", cases.size(),
              nof_reference, shard_index, detections.size() / 3, lowest, highest, std::size(SEQUENCES));
  return 0;
}
