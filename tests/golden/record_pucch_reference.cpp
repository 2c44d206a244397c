// Records the answers of srsRAN-5G-ER's PUCCH format 0 and format 1 receivers for tests/test_pucch.py.  It constructs the
// reference's classes directly -- pucch_detector_format0; dmrs_pucch_processor_format1_impl on port_channel_estimator_average_impl
// (`mean` smoothing, compensate_cfo = false: signal_processor_factories.cpp:123-126) with interpolator_linear_impl and
// time_alignment_estimator_dft_impl over a 4096-point inverse dft_processor_generic_impl; pucch_detector_format1 with
// channel_equalizer_generic_impl(zf), the type upper_phy_factories.cpp:388 hands to the detector factory --, calls them in the
// order and with the field mapping of pucch_processor_impl::process (pucch_processor_impl.cpp:29-128: the BWP offset added to
// both PRBs, beta_pucch 1, estimate dimensions (bwp_start + bwp_size) PRBs x 14 symbols x ports x 1 layer), makes a grid per case
// with a transmitter of its own, and writes inputs and outputs as four .npy files.  Built and run by oracle/recorders.mk,
// against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`, `make -C oracle rerecord-check`; no
// binary or object is committed.  The recipe says why the build is without fused multiply-adds.
//
// Receive ports.  Format 0 is handed the case's port list as it is.  Format 1 is not: pucch_detector_format1 indexes its own
// buffers, the estimate and the noise variances by the port's *identifier* (pucch_detector_format1.cpp:121 and 193-198) where
// the estimator filled them by the port's *position* in the list, so a list other than 0, 1, ..., n - 1 pairs one port's data with
// another port's estimate, or reads beyond the estimate.  A format 1 case with such a list is recorded as what it means --
// receive port i reads grid port ports[i] --: the reference is handed the list 0 .. n - 1 and a grid reader whose port i is grid
// port ports[i].
//
// Cases, in this order.  A *grid group* is one grid and the cases that read it.
//   group 0  the 186 configurations of pucch_configs.json; the two format 1 entries of one "case" share a PRB and a grid (two UEs
//            on other cyclic shifts), a format 0 entry has a grid of its own
//   group 1  the small shapes of small_shapes() below
//   group 2  a zero grid per format (flag 1: the metrics are 0 / 0 and 0 / inf by construction; only exact fields compare)
//   group 3  13 noise-only grids per format, the noise of standard deviation 0.1 ... 10
//   group 4  the grids of test_wrong_cyclic_shift_or_cover_code_is_invalid: flat gains (1, j), noise of 0.05 per component; the
//            case that was sent, then configurations with another cyclic shift or cover code reading the same grid
//
// The transmitter (TS 38.211 Sections 6.3.2.3 and 6.3.2.4, sequences from the reference's low-PAPR collection and
// pucch_orthogonal_sequence, cyclic shifts from its pucch_helper) and the channel of parity_slots() in tests/test_pucch.py: per
// grid port two taps -- the first Rayleigh of mean amplitude a, held above a / 2, delayed by d0 in [0, 8) samples of a 4096-point
// transform; the second of mean amplitude 0.3 a, 5 to 30 samples later --, a CFO of up to 1 % of the spacing for format 1 (a phase
// per symbol start epoch), complex Gaussian noise of unit variance, every component rounded to bf16 (nearest, ties to even).  a^2
// is 160 / (12 data symbols ports) times 0 to 8 dB for format 1, 64 / (symbols ports) times 0 to 6 dB for format 0; two UEs on
// one PRB get a first tap of amplitude a without fading, 8 to 11 dB up.
//
// No fragile decision is recorded: a grid group's channel and noise are drawn again while, for any of its cases,
//   - the decided metric lies in [2, 8] (T = 4: format 1's detection_metric x 4, format 0's 10^(sinr_dB / 10)),
// or, except on noise-only grids,
//   - format 0's best candidate leads the runner-up by less than 2 % (the candidates' metrics evaluated here in double),
//   - a two-bit format 1's statistics |re + im| and |re - im| of the detected symbol are within 2 % of each other (evaluated here
//     in double from what the equaliser returned, through a forwarding channel_equalizer),
//   - the two largest per-port SNRs of a format 1 estimate are within 2 % (the larger decides whose CFO is reported).
//
// Files (case i is row i of `cases` and of `results`):
//   pucch_reference_cases.npy      int32 [n][28]: format, numerology, slot_index, bwp_start_rb, bwp_size_rb, starting_prb,
//                                  second_hop_prb (-1: none), start_symbol_index, nof_symbols, initial_cyclic_shift,
//                                  time_domain_occ, n_id, nof_harq_ack, sr_opportunity, nof_ports, ports[4], offset into grids,
//                                  offset into estimates (-1: format 0), flags (1: ill-conditioned by construction), group, index
//                                  within the group's source (entry of pucch_configs.json, row of small_shapes(), ...), sent ACK
//                                  bits (b0 + 2 b1; SR-only format 1: the bit whose symbol was sent, 0 for a positive SR; -1: this
//                                  case's UE was not sent), sent SR (-1: none), number of draws, 0
//   pucch_reference_grids.npy      uint32 cbf16 words (re in the low half): per grid [nof_ports][nof_symbols][12], row i grid port
//                                  ports[i], column j symbol start + j, the 12 subcarriers of that symbol's PRB (bwp_start +
//                                  starting_prb; bwp_start + second_hop_prb for format 0's second symbol and for format 1's symbols
//                                  from nof_symbols / 2 on).  Every other element of a case's grid (4 ports x 14 x 624) is zero.
//                                  Cases of one grid group have one offset.
//   pucch_reference_results.npy    float64 [n][44]: status (0 unknown, 1 valid, 2 invalid), ACK bit 0, ACK bit 1, SR (NaN: format
//                                  0 on a zero grid, where the reference returns a message whose payload was never written:
//                                  pucch_uci_message.h:60-71), detection_metric (format 1; NaN for format 0), SINR, RSRP, EPRE in
//                                  dB, time alignment in seconds, CFO in Hz (NaN: none); then for format 1 per receive port i
//                                  (NaN beyond the ports and for format 0) noise variance, RSRP, EPRE, SNR, CFO in Hz (NaN: none),
//                                  the time alignment the estimator returned for hop 0 and for hop 1 (NaN: no hop 1) through a
//                                  forwarding time_alignment_estimator, and the time alignment set on the estimate; last the two
//                                  numbers the recorder evaluated in double for the margins above: format 0's two largest
//                                  candidate metrics (the larger first), format 1's |re + im| and |re - im|
//   pucch_reference_estimates.npy  uint32 cbf16 words: per format 1 case [nof_ports][nof_symbols], the estimate on the 12
//                                  subcarriers of the symbol's PRB -- one value; the recorder stops if the 12 differ, or if any
//                                  element of the estimate outside that region was written
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/channel_processors/pucch_detector_format0.h"
#include "lib/phy/upper/channel_processors/pucch_detector_format1.h"
#include "lib/phy/upper/equalization/channel_equalizer_generic_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_collection_impl.h"
#include "lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "lib/phy/upper/signal_processors/pucch/dmrs_pucch_processor_format1_impl.h"
#include "recorder_grid.h"
#include "srsran/phy/upper/pucch_orthogonal_sequence.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>
#include <map>
#include <random>

using namespace srsran;

namespace {

constexpr unsigned GRID_PORTS = 4, GRID_SUBC = 624;
constexpr double   THRESHOLD = 4.0, MARGIN = 0.02;
const double       NaN = std::numeric_limits<double>::quiet_NaN();
using cd = std::complex<double>;

// The grids are word_grid [4][14][624]; for format 1 the reader's port i is grid port ports[i] (word_grid::map).

// Forwards to the reference's time alignment estimator and keeps what it returned, call by call.
class ta_recorder : public time_alignment_estimator
{
  std::unique_ptr<time_alignment_estimator> inner;
  std::vector<double>&                      log;

public:
  ta_recorder(std::unique_ptr<time_alignment_estimator> inner_, std::vector<double>& log_) : inner(std::move(inner_)), log(log_) {}
  time_alignment_measurement estimate(span<const cf_t> symbols, bounded_bitset<max_nof_symbols> mask, subcarrier_spacing scs, double max_ta) override
  {
    const time_alignment_measurement m = inner->estimate(symbols, mask, scs, max_ta);
    log.push_back(m.time_alignment);
    return m;
  }
  time_alignment_measurement estimate(span<const cf_t> symbols, unsigned stride, subcarrier_spacing scs, double max_ta) override
  {
    const time_alignment_measurement m = inner->estimate(symbols, stride, scs, max_ta);
    log.push_back(m.time_alignment);
    return m;
  }
};

// Forwards to the reference's equaliser and keeps the equalised symbols of the last call.
class eq_recorder : public channel_equalizer
{
  std::unique_ptr<channel_equalizer> inner;
  std::vector<cf_t>&                 last;

public:
  eq_recorder(std::unique_ptr<channel_equalizer> inner_, std::vector<cf_t>& last_) : inner(std::move(inner_)), last(last_) {}
  void equalize(span<cf_t> eq_symbols, span<float> eq_noise_vars, const re_buffer_reader<cbf16_t>& ch_symbols, const ch_est_list& ch_estimates,
                span<const float> noise_var_estimates, float tx_scaling) override
  {
    inner->equalize(eq_symbols, eq_noise_vars, ch_symbols, ch_estimates, noise_var_estimates, tx_scaling);
    last.assign(eq_symbols.begin(), eq_symbols.end());
  }
};

struct Cfg {
  int              format, numerology, slot, bwp_start, bwp_size, prb, prb2, start, ns, m0, occ, n_id, nack, sr_opp;
  std::vector<int> ports;
};
struct Entry {
  Cfg cfg;
  int bits; // b0 + 2 b1 of the UE that is sent; -1: nothing is sent for this configuration
  int sr;   // -1: none
  int source;
};
enum Kind { TWO_TAP, ZERO, NOISE_ONLY, FLAT };
struct Group {
  int                group;
  Kind               kind;
  std::vector<Entry> entries;
};

// Symbol offset -> hop (0, 1) of the allocation.
int hop_of(const Cfg& c, int off)
{
  if (c.prb2 < 0) {
    return 0;
  }
  return c.format == 0 ? (off != 0) : (off >= c.ns / 2);
}
int grid_prb(const Cfg& c, int off) { return c.bwp_start + (hop_of(c, off) ? c.prb2 : c.prb); }

struct Sequences {
  low_papr_sequence_generator_impl                   generator;
  std::unique_ptr<low_papr_sequence_collection_impl> collection;
  pucch_helper                                       helper;
  pucch_orthogonal_sequence                          occ;

  static std::array<float, NRE> alphas()
  {
    std::array<float, NRE> a;
    for (unsigned n = 0; n != NRE; ++n) {
      a[n] = TWOPI * static_cast<float>(n) / static_cast<float>(NRE);
    }
    return a;
  }
  Sequences() : helper(std::make_unique<pseudo_random_generator_impl>())
  {
    const std::array<float, NRE> a = alphas();
    collection = std::make_unique<low_papr_sequence_collection_impl>(generator, 1, 0, a);
  }
  std::unique_ptr<low_papr_sequence_collection> make_collection()
  {
    const std::array<float, NRE> a = alphas();
    return std::make_unique<low_papr_sequence_collection_impl>(generator, 1, 0, a);
  }
  // r_uv^alpha(n) of the symbol at offset `off` of the allocation, with m_cs.
  std::vector<cd> r(const Cfg& c, int off, int m_cs)
  {
    const unsigned alpha = helper.get_alpha_index(slot_point(c.numerology, 0, c.slot), cyclic_prefix::NORMAL, c.n_id, c.start + off, c.m0, m_cs);
    span<const cf_t> s = collection->get(c.n_id % 30, 0, alpha);
    std::vector<cd>  out;
    for (const cf_t& v : s) {
      out.emplace_back(v.real(), v.imag());
    }
    return out;
  }
  // Format 1: (is DM-RS, index among the hop's symbols of its kind, their number) of the symbol at offset `off`.
  void layout(const Cfg& c, int off, bool& dmrs, int& m, int& count)
  {
    dmrs  = off % 2 == 0;
    m     = 0;
    count = 0;
    for (int o = 0; o != c.ns; ++o) {
      if (hop_of(c, o) == hop_of(c, off) && (o % 2 == 0) == dmrs) {
        if (o < off) {
          ++m;
        }
        ++count;
      }
    }
  }
  cd w(int count, int i, int m)
  {
    const cf_t v = occ.get_sequence_value(count, i, m);
    return cd(v.real(), v.imag());
  }
};

// TS 38.213 Section 9.2.3 and 9.2.5: format 0's m_cs of the HARQ-ACK bits and a positive SR.
int format0_m_cs(int nack, int bits, int sr)
{
  if (nack == 0) {
    return 0;
  }
  if (nack == 1) {
    return (bits ? 6 : 0) + (sr > 0 ? 3 : 0);
  }
  const int b0 = bits & 1, b1 = bits >> 1;
  const int base = b0 == 0 ? (b1 == 0 ? 0 : 3) : (b1 == 1 ? 6 : 9);
  return base + (sr > 0 ? 1 : 0);
}
std::vector<int> format0_candidates(const Cfg& c)
{
  if (c.nack == 0) {
    return {0};
  }
  if (c.nack == 1) {
    return c.sr_opp ? std::vector<int>{0, 6, 3, 9} : std::vector<int>{0, 6};
  }
  return c.sr_opp ? std::vector<int>{0, 3, 6, 9, 1, 4, 7, 10} : std::vector<int>{0, 3, 6, 9};
}

// The resource elements one UE sends, unit amplitude: x[off][n].
std::vector<std::vector<cd>> transmit(Sequences& seq, const Entry& e)
{
  const Cfg&                   c = e.cfg;
  std::vector<std::vector<cd>> x(c.ns);
  if (c.format == 0) {
    const int m_cs = format0_m_cs(c.nack, e.bits, e.sr);
    for (int off = 0; off != c.ns; ++off) {
      x[off] = seq.r(c, off, m_cs);
    }
    return x;
  }
  // Positive SR alone is one 0 bit; the small shape that sends a 1 there is what the detector calls `unknown`.
  const int    b0 = e.bits & 1, b1 = c.nack == 2 ? (e.bits >> 1) : b0;
  const cd     d  = cd(1 - 2 * b0, 1 - 2 * b1) / std::sqrt(2.0);
  for (int off = 0; off != c.ns; ++off) {
    bool dmrs;
    int  m, count;
    seq.layout(c, off, dmrs, m, count);
    const cd        wv = seq.w(count, c.occ, m);
    std::vector<cd> r  = seq.r(c, off, 0);
    for (cd& v : r) {
      v = dmrs ? wv * v : wv * d * v;
    }
    x[off] = r;
  }
  return x;
}

struct Result {
  double              status, ack[2], sr, metric, sinr, rsrp, epre, ta, cfo;
  double              port[4][8];
  std::vector<uint32_t> estimate; // [ports][ns]
  double              decided;    // the metric the threshold decides on
  double              top[2];     // format 0: the two largest candidate metrics; format 1: the two statistics
  double              snr[2];     // the two largest per-port SNRs
};

double opt(const std::optional<float>& v) { return v.has_value() ? (double)v.value() : NaN; }

struct Reference {
  Sequences                                          seq;
  std::vector<double>                                ta_log;
  std::vector<cf_t>                                  eq_last;
  std::unique_ptr<pucch_detector_format0>            f0;
  std::unique_ptr<dmrs_pucch_processor_format1_impl> estimator;
  std::unique_ptr<pucch_detector_format1>            f1;
  channel_estimate                                   estimates;

  Reference()
  {
    f0 = std::make_unique<pucch_detector_format0>(std::make_unique<pseudo_random_generator_impl>(), seq.make_collection());
    dft_processor::configuration dft_cfg;
    dft_cfg.size = 4096;
    dft_cfg.dir  = dft_processor::direction::INVERSE;
    estimator    = std::make_unique<dmrs_pucch_processor_format1_impl>(
        std::make_unique<pseudo_random_generator_impl>(),
        seq.make_collection(),
        std::make_unique<port_channel_estimator_average_impl>(
            std::make_unique<interpolator_linear_impl>(),
            std::make_unique<ta_recorder>(
                std::make_unique<time_alignment_estimator_dft_impl>(std::make_unique<dft_processor_generic_impl>(dft_cfg)), ta_log),
            port_channel_estimator_fd_smoothing_strategy::mean,
            /*compensate_cfo =*/false));
    f1 = std::make_unique<pucch_detector_format1>(
        seq.make_collection(),
        std::make_unique<pseudo_random_generator_impl>(),
        std::make_unique<eq_recorder>(std::make_unique<channel_equalizer_generic_impl>(channel_equalizer_algorithm_type::zf), eq_last));
  }

  Result format0(word_grid& grid, const Cfg& c)
  {
    grid.map = {0, 1, 2, 3};
    pucch_detector::format0_configuration d;
    d.slot         = slot_point(c.numerology, 0, c.slot);
    d.cp           = cyclic_prefix::NORMAL;
    d.starting_prb = c.prb + c.bwp_start;
    if (c.prb2 >= 0) {
      d.second_hop_prb.emplace(c.prb2 + c.bwp_start);
    }
    d.start_symbol_index   = c.start;
    d.nof_symbols          = c.ns;
    d.initial_cyclic_shift = c.m0;
    d.n_id                 = c.n_id;
    d.nof_harq_ack         = c.nack;
    d.sr_opportunity       = c.sr_opp != 0;
    for (int p : c.ports) {
      d.ports.push_back((uint8_t)p);
    }
    const std::pair<pucch_uci_message, channel_state_information> out = f0->detect(grid, d);
    Result r = {};
    r.status = (double)static_cast<int>(out.first.get_status());
    r.ack[0] = r.ack[1] = r.sr = 0.0;
    r.sinr   = opt(out.second.get_sinr_dB());
    r.rsrp   = opt(out.second.get_rsrp_dB());
    r.epre   = opt(out.second.get_epre_dB());
    r.decided = std::pow(10.0, r.sinr / 10.0);
    if (r.decided > 0) {
      for (int i = 0; i != c.nack; ++i) {
        r.ack[i] = out.first.get_harq_ack_bits()[i];
      }
      if (c.sr_opp) {
        r.sr = out.first.get_sr_bits()[0];
      }
    } else { // the default message: its payload was never written
      r.ack[0] = r.ack[1] = r.sr = NaN;
    }
    r.metric = NaN;
    r.ta     = out.second.get_time_alignment().has_value() ? out.second.get_time_alignment().value().to_seconds() : 0.0;
    r.cfo    = opt(out.second.get_cfo_Hz());
    for (auto& row : r.port) {
      for (double& v : row) {
        v = NaN;
      }
    }
    // The candidates' metrics in double.
    r.top[0] = r.top[1] = 0.0;
    for (int m_cs : format0_candidates(c)) {
      double sum_corr = 0.0, sum_nv = 0.0;
      for (int off = 0; off != c.ns; ++off) {
        const std::vector<cd> s = seq.r(c, off, m_cs);
        for (int p : c.ports) {
          cd     acc = 0.0;
          double pwr = 0.0;
          for (int n = 0; n != 12; ++n) {
            const cf_t y   = grid.at(p, c.start + off, 12 * grid_prb(c, off) + n);
            const cd   lse = cd(y.real(), y.imag()) * std::conj(s[n]);
            acc += lse;
            pwr += std::norm(lse);
          }
          const double corr = std::norm(acc / 12.0), nv = std::max(0.0, pwr / 12.0 - corr);
          sum_corr += corr;
          sum_nv += nv * corr;
        }
      }
      const double metric = sum_nv > 0 ? sum_corr * sum_corr / sum_nv : 0.0;
      if (metric > r.top[0]) {
        r.top[1] = r.top[0];
        r.top[0] = metric;
      } else if (metric > r.top[1]) {
        r.top[1] = metric;
      }
    }
    return r;
  }

  Result format1(word_grid& grid, const Cfg& c)
  {
    const unsigned P = c.ports.size();
    grid.map.assign(c.ports.begin(), c.ports.end());
    grid.map.resize(GRID_PORTS, 0);
    dmrs_pucch_processor::config_t e;
    e.format               = pucch_format::FORMAT_1;
    e.slot                 = slot_point(c.numerology, 0, c.slot);
    e.cp                   = cyclic_prefix::NORMAL;
    e.start_symbol_index   = c.start;
    e.nof_symbols          = c.ns;
    e.starting_prb         = c.prb + c.bwp_start;
    e.intra_slot_hopping   = c.prb2 >= 0;
    e.second_hop_prb       = c.prb2 >= 0 ? c.prb2 + c.bwp_start : e.starting_prb;
    e.initial_cyclic_shift = c.m0;
    e.time_domain_occ      = c.occ;
    e.n_id                 = c.n_id;
    for (unsigned i = 0; i != P; ++i) {
      e.ports.push_back((uint8_t)i);
    }
    e.group_hopping   = pucch_group_hopping::NEITHER;
    e.nof_prb         = 0;
    e.n_id_0          = 0;
    e.additional_dmrs = false;

    channel_estimate::channel_estimate_dimensions dims;
    dims.nof_prb       = c.bwp_start + c.bwp_size;
    dims.nof_symbols   = 14;
    dims.nof_rx_ports  = P;
    dims.nof_tx_layers = 1;
    estimates.resize(dims);
    const cbf16_t untouched(7.0F, -7.0F);
    for (unsigned i = 0; i != P; ++i) {
      span<cbf16_t> path = estimates.get_path_ch_estimate(i);
      std::fill(path.begin(), path.end(), untouched);
    }
    ta_log.clear();
    estimator->estimate(estimates, grid, e);

    pucch_detector::format1_configuration d;
    d.slot         = e.slot;
    d.cp           = cyclic_prefix::NORMAL;
    d.starting_prb = c.prb + c.bwp_start;
    if (c.prb2 >= 0) {
      d.second_hop_prb.emplace(c.prb2 + c.bwp_start);
    }
    d.start_symbol_index = c.start;
    d.nof_symbols        = c.ns;
    d.group_hopping      = pucch_group_hopping::NEITHER;
    for (unsigned i = 0; i != P; ++i) {
      d.ports.push_back((uint8_t)i);
    }
    d.beta_pucch           = 1.0F;
    d.time_domain_occ      = c.occ;
    d.initial_cyclic_shift = c.m0;
    d.n_id                 = c.n_id;
    d.nof_harq_ack         = c.nack;
    const pucch_detector::pucch_detection_result det = f1->detect(grid, estimates, d);
    channel_state_information                    csi;
    estimates.get_channel_state_information(csi);

    Result r = {};
    r.status = (double)static_cast<int>(det.uci_message.get_status());
    for (int i = 0; i != c.nack; ++i) {
      r.ack[i] = det.uci_message.get_harq_ack_bits()[i];
    }
    r.metric  = det.detection_metric;
    r.decided = (double)det.detection_metric * THRESHOLD;
    r.sinr    = opt(csi.get_sinr_dB());
    r.rsrp    = opt(csi.get_rsrp_dB());
    r.epre    = opt(csi.get_epre_dB());
    r.ta      = csi.get_time_alignment().value().to_seconds();
    r.cfo     = opt(csi.get_cfo_Hz());
    const unsigned hops = c.prb2 >= 0 ? 2 : 1;
    if (ta_log.size() != P * hops) {
      std::fprintf(stderr, "%zu time alignment calls for %u ports and %u hops\n", ta_log.size(), P, hops);
      std::exit(1);
    }
    for (auto& row : r.port) {
      for (double& v : row) {
        v = NaN;
      }
    }
    r.snr[0] = r.snr[1] = 0.0;
    for (unsigned i = 0; i != P; ++i) {
      r.port[i][0] = estimates.get_noise_variance(i);
      r.port[i][1] = estimates.get_rsrp(i);
      r.port[i][2] = estimates.get_epre(i);
      r.port[i][3] = estimates.get_snr(i);
      r.port[i][4] = opt(estimates.get_cfo_Hz(i));
      r.port[i][5] = ta_log[i * hops];
      r.port[i][6] = hops == 2 ? ta_log[i * hops + 1] : NaN;
      r.port[i][7] = estimates.get_time_alignment(i).to_seconds();
      const double s = r.port[i][3];
      if (s > r.snr[0]) {
        r.snr[1] = r.snr[0];
        r.snr[0] = s;
      } else if (s > r.snr[1]) {
        r.snr[1] = s;
      }
    }
    // The estimate: one value on the 12 subcarriers of every symbol's PRB, nothing else written.
    const uint32_t same = word_of(untouched);
    for (unsigned i = 0; i != P; ++i) {
      for (int l = 0; l != 14; ++l) {
        span<const cbf16_t> row    = estimates.get_symbol_ch_estimate(l, i);
        const bool          inside = l >= c.start && l < c.start + c.ns;
        const unsigned      k0     = inside ? 12 * grid_prb(c, l - c.start) : 0;
        for (unsigned k = 0; k != row.size(); ++k) {
          const bool in_region = inside && k >= k0 && k < k0 + 12;
          if (in_region ? word_of(row[k]) != word_of(row[k0]) : word_of(row[k]) != same) {
            std::fprintf(stderr, "estimate: port %u symbol %d subcarrier %u is not what the layout says\n", i, l, k);
            std::exit(1);
          }
        }
        if (inside) {
          r.estimate.push_back(word_of(row[k0]));
        }
      }
    }
    // The detected symbol in double from what the equaliser returned: sum of eq conj(w) conj(r) over the data symbols.
    cd       detected = 0.0;
    unsigned at       = 0;
    for (int off = 1; off < c.ns; off += 2) {
      bool dmrs;
      int  m, count;
      seq.layout(c, off, dmrs, m, count);
      const cd              wv = std::conj(seq.w(count, c.occ, m));
      const std::vector<cd> s  = seq.r(c, off, 0);
      for (int n = 0; n != 12; ++n, ++at) {
        detected += cd(eq_last[at].real(), eq_last[at].imag()) * wv * std::conj(s[n]);
      }
    }
    if (at != eq_last.size()) {
      std::fprintf(stderr, "%zu equalised symbols, %u expected\n", eq_last.size(), at);
      std::exit(1);
    }
    r.top[0] = std::abs(detected.real() + detected.imag());
    r.top[1] = std::abs(detected.real() - detected.imag());
    return r;
  }
};

// {format, numerology, slot, bwp_start, bwp_size, prb, prb2, start, symbols, m0, occ, n_id, ACK bits, SR opportunity}, ports.
std::vector<Group> small_shapes()
{
  std::vector<Group> out;
  int                row = 0;
  auto add = [&](Cfg c, int bits, int sr) { out.push_back({1, TWO_TAP, {{c, bits, sr, row++}}}); };
  // Format 0: every candidate of each of the five tables, over the shapes.
  const std::vector<Cfg> f0 = {
      {0, 0, 3, 0, 52, 7, -1, 13, 1, 4, 0, 500, 0, 1, {2}},            // 1 symbol on 1 port, last symbol of the slot
      {0, 0, 0, 1, 51, 0, -1, 5, 2, 0, 0, 0, 0, 1, {0, 1}},            // 2 symbols, no hop, PRB 0 of a BWP from 1, n_id 0
      {0, 1, 19, 1, 51, 50, 3, 12, 2, 11, 0, 1023, 0, 1, {3, 1, 0, 2}}, // hop, last PRB, numerology 1 slot 19, n_id 1023, 4 ports
      {0, 0, 9, 3, 40, 39, 0, 0, 2, 7, 0, 77, 0, 1, {1, 3}},           // hop from the last PRB of the BWP to its first
  };
  int k = 0;
  const int tables[5][2] = {{0, 1}, {1, 0}, {2, 0}, {1, 1}, {2, 1}};
  for (const auto& t : tables) {
    const int nack = t[0], sr_opp = t[1];
    for (int sr = 0; sr <= (sr_opp && nack ? 1 : 0); ++sr) {
      for (int bits = 0; bits != (1 << nack); ++bits) {
        Cfg c    = f0[k++ % f0.size()];
        c.nack   = nack;
        c.sr_opp = sr_opp;
        add(c, bits, sr_opp ? (nack ? sr : 1) : -1);
      }
    }
  }
  // Format 1.
  const std::vector<Cfg> f1 = {
      {1, 0, 3, 0, 52, 5, -1, 0, 4, 4, 1, 500, 1, 0, {0}},              // 4 symbols, no hop, largest OCC (1 of 2)
      {1, 0, 3, 0, 52, 5, 20, 0, 4, 4, 0, 500, 2, 0, {0, 1}},           // 4 symbols, hop: one DM-RS symbol per hop, no CFO
      {1, 0, 4, 1, 51, 0, 50, 2, 5, 9, 0, 0, 1, 0, {1, 3}},             // 5 symbols, hop 2 + 3: CFO from the second hop only
      {1, 0, 5, 1, 51, 50, -1, 10, 4, 0, 1, 1023, 0, 0, {2}},           // 4 symbols from symbol 10, last PRB, SR only
      {1, 0, 6, 0, 52, 11, -1, 0, 14, 3, 6, 301, 2, 0, {0, 1, 2, 3}},   // 14 symbols, no hop, OCC 6 of 7
      {1, 0, 7, 0, 52, 11, 30, 0, 14, 3, 2, 301, 1, 0, {3, 1, 0, 2}},   // 14 symbols, hop, OCC 2 of 3, permuted ports
      {1, 1, 19, 1, 51, 50, 0, 0, 14, 6, 0, 1023, 0, 0, {1, 0}},        // numerology 1 slot 19, hop from the last PRB to PRB 0
      {1, 0, 0, 1, 51, 0, -1, 1, 5, 2, 1, 0, 2, 0, {3}},                // 5 symbols, no hop, OCC 1 of 2
      {1, 0, 1, 0, 52, 8, -1, 3, 6, 1, 2, 45, 1, 0, {0, 2}},            // 6 symbols, OCC 2 of 3
      {1, 0, 2, 0, 52, 8, 9, 2, 6, 1, 0, 45, 2, 0, {2, 0}},             // 6 symbols, hop 3 + 3: hops of 2 and 1 DM-RS symbols
      {1, 0, 8, 0, 52, 17, -1, 0, 7, 5, 2, 600, 0, 0, {0, 1, 2, 3}},    // 7 symbols, OCC 2 of 3
      {1, 0, 9, 0, 52, 17, 18, 0, 8, 5, 1, 600, 2, 0, {1}},             // 8 symbols, hop, OCC 1 of 2
      {1, 0, 2, 0, 52, 25, -1, 0, 8, 10, 3, 999, 1, 0, {1, 2}},         // 8 symbols, OCC 3 of 4
      {1, 0, 3, 0, 52, 25, 26, 5, 9, 10, 1, 999, 2, 0, {0, 3}},         // 9 symbols, hop 4 + 5, OCC 1 of 2
      {1, 1, 11, 0, 52, 33, -1, 1, 10, 8, 4, 123, 2, 0, {2, 3}},        // 10 symbols, OCC 4 of 5
      {1, 0, 4, 0, 52, 33, -1, 0, 12, 8, 5, 123, 1, 0, {0}},            // 12 symbols, OCC 5 of 6
      {1, 0, 5, 0, 52, 40, 2, 0, 13, 7, 2, 64, 2, 0, {0, 1, 2, 3}},     // 13 symbols, hop 6 + 7, OCC 2 of 3
      {1, 1, 0, 0, 52, 40, 41, 0, 12, 7, 2, 64, 0, 0, {2, 1}},          // 12 symbols, hop, OCC 2 of 3, SR only
  };
  for (const Cfg& c : f1) {
    for (int bits = 0; bits != (1 << c.nack); ++bits) {
      if (c.nack == 2 && c.ns != 14 && c.ns != 4 && bits != ((c.ns + c.m0) & 3)) {
        continue; // all four symbols on the 4- and 14-symbol shapes, one elsewhere
      }
      add(c, bits, -1);
    }
  }
  // SR only with the symbol of a 1 bit, which no UE sends: above the threshold the detector's status is `unknown`.
  add({1, 0, 6, 0, 52, 21, -1, 0, 6, 5, 1, 210, 0, 0, {0, 1}}, 1, -1);
  return out;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s pucch_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream     in(argv[1]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  const std::string text = buffer.str();
  const std::string dir  = argv[2];

  std::vector<Group>   groups;
  std::map<int, size_t> by_case;
  const std::regex     object("\\{\"format\"[^}]*\\}");
  int                  index = 0;
  for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it, ++index) {
    const std::string o  = it->str();
    const int         mu = json_int(o, "numerology");
    Cfg c = {json_int(o, "format"), mu, json_int(o, "slot_count") % (10 << mu), json_int(o, "bwp_start_rb"), json_int(o, "bwp_size_rb"),
             json_int(o, "starting_prb"), json_int(o, "second_hop_prb", -1), json_int(o, "start_symbol_index"), json_int(o, "nof_symbols"),
             json_int(o, "initial_cyclic_shift"), json_int(o, "time_domain_occ", 0), json_int(o, "n_id"), json_int(o, "nof_harq_ack"),
             json_int(o, "sr_opportunity", 0), json_list(o, "ports")};
    const std::vector<int> ack = json_list(o, "ack_bits");
    const Entry e = {c, (ack.size() > 0 ? ack[0] : 0) + (ack.size() > 1 ? 2 * ack[1] : 0), json_int(o, "sr", -1), index};
    if (c.format == 1) {
      const int id = json_int(o, "case");
      if (by_case.count(id)) {
        groups[by_case[id]].entries.push_back(e);
        continue;
      }
      by_case[id] = groups.size();
    }
    groups.push_back({0, TWO_TAP, {e}});
  }
  const size_t nof_fixture = index;
  for (const Group& g : small_shapes()) {
    groups.push_back(g);
  }
  std::mt19937                          rng(20240705);
  std::normal_distribution<double>      normal(0.0, 1.0);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  const Cfg zero0 = {0, 0, 3, 0, 52, 3, -1, 5, 2, 0, 0, 0, 2, 1, {0, 1}}, zero1 = {1, 0, 3, 0, 52, 3, 20, 0, 14, 0, 0, 0, 2, 0, {0, 1, 2, 3}};
  groups.push_back({2, ZERO, {{zero0, -1, -1, 0}}});
  groups.push_back({2, ZERO, {{zero1, -1, -1, 1}}});
  for (int k = 0; k != 26; ++k) { // noise only: the shapes drawn here
    const std::vector<int> ports = k % 3 == 0 ? std::vector<int>{0} : k % 3 == 1 ? std::vector<int>{1, 2} : std::vector<int>{0, 1, 2, 3};
    auto                   pick  = [&](int n) { return (int)(rng() % (unsigned)n); };
    Cfg                    c;
    if (k % 2) {
      const int ns = 4 + pick(11), hop = pick(2);
      c = {1, 0, pick(10), 0, 52, pick(52), hop ? pick(52) : -1, pick(std::min(10, 14 - ns) + 1), ns, pick(12), 0, pick(1024), pick(3), 0, ports};
    } else {
      const int nack = pick(3), ns = 1 + pick(2);
      c = {0, 0, pick(10), 0, 52, pick(52), -1, pick(15 - ns), ns, pick(12), 0, pick(1024), nack, nack == 0 ? 1 : pick(2), ports};
    }
    groups.push_back({3, NOISE_ONLY, {{c, -1, -1, k}}});
  }
  {
    const Cfg c = {1, 0, 2, 0, 52, 9, -1, 0, 14, 3, 1, 301, 1, 0, {0, 1}};
    Group     g = {4, FLAT, {{c, 1, -1, 0}}};
    Cfg       o = c;
    o.m0        = 4;
    g.entries.push_back({o, -1, -1, 1});
    o.m0 = 9;
    g.entries.push_back({o, -1, -1, 2});
    o     = c;
    o.occ = 0;
    g.entries.push_back({o, -1, -1, 3});
    o.occ = 5;
    g.entries.push_back({o, -1, -1, 4});
    groups.push_back(g);
    const Cfg f = {0, 0, 2, 0, 52, 9, -1, 12, 2, 3, 0, 301, 1, 0, {0, 1}};
    Group     h = {4, FLAT, {{f, 1, -1, 5}}};
    o           = f;
    o.m0        = 4;
    h.entries.push_back({o, -1, -1, 6});
    groups.push_back(h);
  }

  Reference             ref;
  std::vector<int32_t>  rows;
  std::vector<uint32_t> grids, estimates;
  std::vector<double>   results;
  size_t                nof_cases = 0, nof_ta = 0, nonzero_ta = 0, draws_total = 0;
  for (size_t ig = 0; ig != groups.size(); ++ig) {
    const Group& g = groups[ig];
    const Cfg&   c = g.entries[0].cfg;
    for (const Entry& e : g.entries) { // one region per group
      const Cfg& o = e.cfg;
      if (o.ports != c.ports || o.start != c.start || o.ns != c.ns || o.prb != c.prb || o.prb2 != c.prb2 || o.bwp_start != c.bwp_start ||
          o.format != c.format || o.numerology != c.numerology || GRID_SUBC < 12 * (unsigned)(o.bwp_start + o.bwp_size)) {
        std::fprintf(stderr, "group %zu: its cases do not share a region\n", ig);
        return 1;
      }
    }
    const std::vector<double> ep = epochs(c.numerology);
    word_grid                 grid(GRID_PORTS, GRID_SUBC);
    std::vector<Result>       res;
    unsigned                  draws = 0;
    bool                      fragile;
    do {
      ++draws;
      std::vector<cd> acc(GRID_PORTS * 14 * 12, 0.0); // [grid port][offset][n]
      const unsigned  sent = std::count_if(g.entries.begin(), g.entries.end(), [](const Entry& e) { return e.bits >= 0; });
      for (const Entry& e : g.entries) {
        if (e.bits < 0) {
          continue;
        }
        const std::vector<std::vector<cd>> x = transmit(ref.seq, e);
        const unsigned                     P = c.ports.size();
        std::vector<cd>                    g0(GRID_PORTS), g1(GRID_PORTS, 0.0);
        double                             d0 = 0.0, d1 = 0.0, cfo = 0.0;
        if (g.kind == FLAT) {
          g0 = {cd(1, 0), cd(0, 1), 0.0, 0.0};
        } else {
          const bool   shared = sent > 1;
          const double floor_db =
              c.format == 1 ? 10 * std::log10(160.0 / (12 * (c.ns / 2) * P)) : 10 * std::log10(64.0 / (c.ns * P));
          const double snr_db = floor_db + (shared ? 8 + 3 * uniform(rng) : (c.format == 1 ? 8 : 6) * uniform(rng));
          const double amp    = std::pow(10.0, snr_db / 20);
          d0                  = 8 * uniform(rng);
          d1                  = d0 + 5 + 25 * uniform(rng);
          cfo                 = c.format == 1 ? 0.02 * uniform(rng) - 0.01 : 0.0;
          for (unsigned p = 0; p != GRID_PORTS; ++p) {
            cd a = amp * cd(normal(rng), normal(rng)) / std::sqrt(2.0);
            if (shared) {
              a = std::polar(amp, std::arg(a));
            } else if (std::abs(a) < 0.5 * amp) {
              a = std::polar(0.5 * amp, std::arg(a));
            }
            g0[p] = a;
            g1[p] = 0.3 * amp * cd(normal(rng), normal(rng)) / std::sqrt(2.0);
          }
        }
        for (unsigned p = 0; p != GRID_PORTS; ++p) {
          for (int off = 0; off != c.ns; ++off) {
            const cd rot = std::polar(1.0, 2 * M_PI * cfo * ep[c.start + off]);
            for (int n = 0; n != 12; ++n) {
              const double k = 12 * grid_prb(c, off) + n;
              acc[(p * 14 + off) * 12 + n] +=
                  (g0[p] * std::polar(1.0, -2 * M_PI * k * d0 / 4096.0) + g1[p] * std::polar(1.0, -2 * M_PI * k * d1 / 4096.0)) * rot * x[off][n];
            }
          }
        }
      }
      double sigma = std::sqrt(0.5); // per component
      if (g.kind == NOISE_ONLY) {
        sigma = 0.1 + 9.9 * uniform(rng);
      } else if (g.kind == FLAT) {
        sigma = 0.05;
      } else if (g.kind == ZERO) {
        sigma = 0.0;
      }
      for (int p : c.ports) {
        for (int off = 0; off != c.ns; ++off) {
          for (int n = 0; n != 12; ++n) {
            const cd v = acc[(p * 14 + off) * 12 + n] + sigma * cd(normal(rng), normal(rng));
            grid.set(p, c.start + off, 12 * grid_prb(c, off) + n, (float)v.real(), (float)v.imag());
          }
        }
      }
      res.clear();
      fragile = false;
      for (const Entry& e : g.entries) {
        const Result r = e.cfg.format == 0 ? ref.format0(grid, e.cfg) : ref.format1(grid, e.cfg);
        res.push_back(r);
        if (g.kind == ZERO) {
          continue;
        }
        fragile = fragile || (r.decided >= THRESHOLD / 2 && r.decided <= 2 * THRESHOLD);
        if (g.kind == NOISE_ONLY) {
          continue;
        }
        const double hi = std::max(r.top[0], r.top[1]), lo = std::min(r.top[0], r.top[1]);
        if (e.cfg.format == 0 ? format0_candidates(e.cfg).size() > 1 : e.cfg.nack == 2) {
          fragile = fragile || (hi - lo < MARGIN * hi);
        }
        if (e.cfg.format == 1 && e.cfg.ports.size() > 1) {
          fragile = fragile || (r.snr[0] - r.snr[1] < MARGIN * r.snr[0]);
        }
      }
    } while (fragile && draws != 10000);
    if (fragile) {
      std::fprintf(stderr, "group %zu: every draw fragile\n", ig);
      return 1;
    }
    draws_total += draws;
    const size_t grid_offset = grids.size();
    for (int p : c.ports) {
      for (int off = 0; off != c.ns; ++off) {
        for (int n = 0; n != 12; ++n) {
          grids.push_back(grid.word(p, c.start + off, 12 * grid_prb(c, off) + n));
        }
      }
    }
    for (size_t ie = 0; ie != g.entries.size(); ++ie) {
      const Entry&  e = g.entries[ie];
      const Cfg&    o = e.cfg;
      const Result& r = res[ie];
      const int     P = o.ports.size();
      const int32_t row[28] = {o.format, o.numerology, o.slot, o.bwp_start, o.bwp_size, o.prb, o.prb2, o.start, o.ns, o.m0, o.occ, o.n_id,
                               o.nack, o.sr_opp, P, o.ports[0], P > 1 ? o.ports[1] : 0, P > 2 ? o.ports[2] : 0, P > 3 ? o.ports[3] : 0,
                               (int)grid_offset, o.format == 1 ? (int)estimates.size() : -1, g.kind == ZERO ? 1 : 0, g.group, e.source,
                               e.bits, e.sr, (int)draws, 0};
      rows.insert(rows.end(), row, row + 28);
      estimates.insert(estimates.end(), r.estimate.begin(), r.estimate.end());
      double out[44] = {r.status, r.ack[0], r.ack[1], r.sr, r.metric, r.sinr, r.rsrp, r.epre, r.ta, r.cfo};
      for (int i = 0; i != 4; ++i) {
        for (int j = 0; j != 8; ++j) {
          out[10 + 8 * i + j] = r.port[i][j];
        }
      }
      out[42] = r.top[0];
      out[43] = r.top[1];
      results.insert(results.end(), out, out + 44);
      ++nof_cases;
      if (o.format == 1) {
        for (int i = 0; i != P; ++i) {
          for (int j = 5; j != 8; ++j) {
            if (!std::isnan(r.port[i][j])) {
              ++nof_ta;
              nonzero_ta += r.port[i][j] != 0.0;
            }
          }
        }
        nonzero_ta += r.ta != 0.0;
      }
    }
  }
  write_npy(dir + "/pucch_reference_cases.npy", "<i4", rows, 28);
  write_npy(dir + "/pucch_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pucch_reference_results.npy", "<f8", results, 44);
  write_npy(dir + "/pucch_reference_estimates.npy", "<u4", estimates, 0);
  std::printf("%zu cases (%zu of the reference's) in %zu grids, %zu draws; %zu grid words, %zu estimate words; %zu of %zu format 1 time "
              "alignments are not 0\n",
              nof_cases, nof_fixture, groups.size(), draws_total, grids.size(), estimates.size(), nonzero_ta, nof_ta);
  return 0;
}
