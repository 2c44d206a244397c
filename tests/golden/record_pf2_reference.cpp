// Records the answers of srsRAN-5G-ER's PUCCH format 2 receiver for tests/test_pucch_format2.py.  It constructs the reference's
// classes directly, in the composition of the factories -- dmrs_pucch_processor_format2_impl over
// port_channel_estimator_average_impl (`filter` smoothing, compensate_cfo = true: the default argument, which
// signal_processor_factories.cpp:129-132 leaves alone) with interpolator_linear_impl and time_alignment_estimator_dft_impl over a
// 4096-point inverse dft_processor_generic_impl; pucch_demodulator_impl with channel_equalizer_generic_impl(zf), the reference's
// demodulation mapper and pseudo_random_generator_impl; uci_decoder_impl with the short-block detector and the polar chain, as
// record_uci_reference.cpp builds it --, and calls them in the order and with the field mapping of
// pucch_processor_impl::process(grid, format2_configuration) (pucch_processor_impl.cpp:131-215): the estimate resized to
// (bwp_start + bwp_size) PRB x 14 symbols x ports x 1 layer, the BWP offset added to the PRB for both the estimator and the
// demodulator, get_channel_state_information after the estimate, the decoder on the demodulator's soft bits.  It makes a grid per
// group of cases with a transmitter of its own and writes inputs and outputs as one .json and seven .npy files.  Built and run by
// oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`,
// `make -C oracle rerecord-check`; no binary or object is committed.  The recipe says why the build is without fused
// multiply-adds and why the equaliser is the scalar one.
//
// Three forwarding objects.  The forwarding interpolator keeps its float32 input per port: the smoothed pilots, after LS, CFO
// derotation, averaging, virtual pilots and the FIR and before any bf16 rounding; it stops unless it is asked for offset 1 and
// stride 3.  The forwarding time_alignment_estimator keeps what it was handed and what it answered; the recorder stops unless it
// was handed the smoothed pilots, bit for bit, on the allocation's pilot subcarriers.  The forwarding channel_equalizer keeps the
// equalised symbols, their noise variances and the per-port noise variances it was handed.
//
// Receive ports.  The reference's format 2 path mixes identifier and position, as its format 1 detector does: the estimator reads
// grid port ports[i] for receive port i (est_cfg.rx_ports, port_channel_estimator_average_impl.cpp:443) and fills the estimate
// by the port's *position*, while pucch_demodulator_impl::get_data_re_ests reads grid port i (pucch_demodulator_impl.cpp:119-133),
// so a list other than 0, 1, ..., n - 1 pairs one port's data with another port's estimate.  A case with such a list is recorded as
// what it means -- receive port i reads grid port ports[i] --: the reference is handed the list 0 .. n - 1 and a grid reader whose
// port i is grid port ports[i].
//
// Cases, in this order.  A *group* is one grid and the cases that read it.
//   group 0  the 196 configurations fixture_cfgs() of the test file derives from pf2_configs.json, in its order: the 144
//            `processor` entries; the 48 `demodulator` entries (PRB first_prb of a BWP of grid_nof_prb PRBs from 0, 4 HARQ-ACK
//            bits, the other fields at their defaults: numerology 0, slot 0, n_id_0 0); the 4 `dmrs` entries that do not hop (a
//            BWP of 275 PRBs from 0, rnti 1, 4 HARQ-ACK bits).  The grid has max(rx_ports) + 1 ports and grid_nof_prb (dmrs: 275) PRBs.
//   group 1  small_shapes(): the ten SHAPES of the test file, field for field, on its grid of 4 ports x 52 PRB, then a 16 PRB x 1
//            symbol and a 2 PRB x 2 symbol case on a single port
//   group 2  a zero grid read with A = 3 and with A = 12 (flag 1: the measurements are 0 / 0 by construction; only exact fields
//            compare)
//   group 3  16 noise-only grids, the noise of standard deviation 10^(-3 + 4 k / 15) per component, k = 0 .. 15: 1, 2 and 4 ports,
//            both symbol counts, 1, 2, 3 and 16 PRB, A <= 11 for even k and A >= 12 for odd k
//   group 4  three shapes of group 1 with A >= 12 sent again, each grid read by the configuration that was sent and then with
//            rnti ^ 1, with n_id ^ 1 and with n_id_0 ^ 1
//
// The transmitter.  Payload bits from the seeded generator; encoded with the reference's short_block_encoder_impl (A <= 11) or
// its CRC, polar allocator, encoder and rate matcher (A >= 12), as record_uci_reference.cpp makes its soft bits; scrambled with
// the reference's generator at rnti 2^15 + n_id; QPSK ((1 - 2 b0) + j (1 - 2 b1)) / sqrt(2) on the resource elements with k mod 3
// != 1, symbol by symbol, subcarriers ascending; on k mod 3 == 1 the DM-RS of TS 38.211 Section 6.4.1.3.2: r_l(m) of the
// reference's generator at c_init = (2^17 (14 n_slot + l + 1)(2 n_id_0 + 1) + 2 n_id_0) mod 2^31, generated from m = 0 -- subcarrier
// 0 of the grid -- and read at m = 4 n_prb + j, so nothing here advances a generator.
//
// The channel is that of record_pucch_reference.cpp.  Per grid port two taps -- the first Rayleigh of mean amplitude a, held above
// a / 2, delayed by d0 in [0, 8) samples of a 4096-point transform; the second of mean amplitude 0.3 a, 5 to 30 samples later --, a
// CFO of up to 1 % of the spacing (a phase per symbol start epoch, epochs() of recorder_grid.h), complex Gaussian noise of unit
// variance, every component rounded to bf16 (nearest, ties to even).  a^2 is, per port, a floor of 16 dB plus 0 to
// 8 dB: the weakest case, the (32, 25) polar code of A = 19 on one port, needs about 10 dB (LINK_SNR_DB of the test file), and the
// first tap may lie 6 dB below a.
//
// No fragile decision is recorded: a group's channel, delays, CFO and noise are drawn again, at most 10000 times, while for any of
// its cases
//   - time alignment: the best of the 288 searched powers (bins [0, 144) and [3952, 4096) of the 4096-point inverse transform of the
//     smoothed pilots, evaluated here in double, per port) leads the runner-up, by (best - runner-up) / best, by less than
//     min(2 %, c / 2), c = (2 pi / 4096)^2 Var(pilot subcarrier numbers): the rule of record_pusch_chest_reference.cpp, whose header
//     gives its reason.  The recorder stops if the reference's bin is not the one found in double.  Noise-only and zero grids are
//     exempt; their lead is recorded anyway.
//   - best port: the two largest per-port SNRs are within 2 % of each other (MARGIN of record_pucch_reference.cpp; the larger
//     decides whose time alignment and CFO are reported).  Zero grids are exempt: every port has the SNR 1000 there.
//   - short block, A <= 11: the detection metric, evaluated here in double from the reference's soft bits (the expressions of
//     short_block_detector_impl.cpp:97-144, the codewords from short_block_encoder_impl), lies in [T / 2, 2 T], T the threshold of
//     short_block_detector_impl.cpp:194-197.  On 1 PRB x 1 symbol (16 soft bits) the metric cannot exceed 31, which is below 2 T
//     from A = 5 on: there the band is [T / 2, (T + 31) / 2] (band_end() below).  The recorder stops if its best codeword is not the
//     message the reference returned.
//   - a case whose UE was sent: the reference does not return the sent message with status `valid`.
//
// The recorder stops if any element of the estimate outside the allocation's region changed (it marks the estimate beforehand),
// but for this: with a CFO -- two symbols -- the reference rotates the whole row of both symbols, so a subcarrier outside the
// allocation comes back as its old content rotated, one value of the mark's magnitude per row.  The library leaves those alone.  It
// also stops unless the equaliser returned 8 nof_prb nof_symbols symbols.
//
// Every file stays under 1 MB (SIZE_CAP of the tests) with all 196 entries of group 0: none is dropped.
//
// Files (offsets in elements of the named file; case i is entry i of `cases`):
//   pf2_reference_cases.json      per case: numerology, slot_index, bwp_size_rb, bwp_start_rb, starting_prb, nof_prb,
//                                 start_symbol_index, nof_symbols, rnti, n_id, n_id_0, nof_harq_ack, nof_sr, nof_csi_part1,
//                                 nof_csi_part2, rx_ports, grid_nof_ports, grid_nof_prb (the grid the case is read from), group,
//                                 source (index within the group's source: entry of fixture_cfgs(), row of small_shapes(), ...), flags
//                                 (1: zero grid), draws, A, sent (1: this case's UE was sent), snr_db (per grid port named by
//                                 rx_ports, in its order), delay (d0), delay2 (d1), cfo (of the spacing), sigma (per component),
//                                 grid_off, pilot_off, est_off, eq_off, llr_off, msg_off, res_row
//   pf2_reference_grids.npy       uint32 cbf16 words (re in the low half): per grid [P][nof_symbols][12 nof_prb], row i what
//                                 receive port i reads (grid port rx_ports[i]), the allocation's symbols and subcarriers ascending.
//                                 Every other element of the case's grid is zero.  Cases of one group have one offset.
//   pf2_reference_pilots.npy      complex64: per case [P][4 nof_prb], the smoothed pilots
//   pf2_reference_estimates.npy   uint32 cbf16 words: per case [P][nof_symbols][12 nof_prb], the estimate on the allocation
//   pf2_reference_eq.npy          float32 [rows][3]: per case 8 nof_prb nof_symbols rows of (re, im) of the equalised symbol and its
//                                 noise variance, in the order the equaliser returned them
//   pf2_reference_llr.npy         int8: per case [16 nof_prb nof_symbols], the descrambled soft bits the decoder read
//   pf2_reference_messages.npy    uint8: per case the A sent bits (only where sent is 1), then the A bits decode() left in a buffer
//                                 that held 0 in every byte
//   pf2_reference_results.npy     float64 [n][48]: decoder status (1 valid, 2 invalid); the short-block metric in double (NaN for
//                                 A >= 12 and where every soft bit is 0); SINR, RSRP, EPRE in dB; time alignment in seconds; CFO in
//                                 Hz (NaN: none); the first port of the largest SNR; then per receive port i (NaN beyond the ports)
//                                 noise variance, RSRP, EPRE, SNR, CFO in Hz (NaN: none), the time alignment the forwarding
//                                 estimator answered in seconds, that as a bin, best and runner-up power in double, the lead
//                                 asked for
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/support/interpolator/interpolator_linear_impl.h"
#include "lib/phy/support/time_alignment_estimator/time_alignment_estimator_dft_impl.h"
#include "lib/phy/upper/channel_coding/crc_calculator_generic_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_allocator_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_code_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_deallocator_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_decoder_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_encoder_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_rate_dematcher_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_rate_matcher_impl.h"
#include "lib/phy/upper/channel_coding/short/short_block_detector_impl.h"
#include "lib/phy/upper/channel_coding/short/short_block_encoder_impl.h"
#include "lib/phy/upper/channel_modulation/demodulation_mapper_impl.h"
#include "lib/phy/upper/channel_processors/pucch_demodulator_impl.h"
#include "lib/phy/upper/channel_processors/uci/uci_decoder_impl.h"
#include "lib/phy/upper/equalization/channel_equalizer_generic_impl.h"
#include "lib/phy/upper/sequence_generators/pseudo_random_generator_impl.h"
#include "lib/phy/upper/signal_processors/port_channel_estimator_average_impl.h"
#include "lib/phy/upper/signal_processors/pucch/dmrs_pucch_processor_format2_impl.h"
#include "recorder_grid.h"
#include "srsran/ran/uci/uci_info.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <limits>
#include <random>

using namespace srsran;

namespace {

constexpr double MARGIN = 0.02;
constexpr int    TA_WINDOW = 144, DFT = 4096, COLS = 48;
constexpr double THRESHOLDS[11] = {0, 0, 12, 14, 16, 18, 20, 22, 24, 26, 29}; // short_block_detector_impl.cpp:194-197, by A - 1
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
    if (cfg.offset != 1 || cfg.stride != 3) {
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
    std::fprintf(stderr, "time alignment: the strided call is not the port estimator's\n");
    std::exit(1);
  }
};

// Forwards to the reference's equaliser and keeps what the last call returned and the noise variances it was handed.
struct eq_call {
  std::vector<cf_t>  symbols;
  std::vector<float> noise_vars, port_noise_vars;
};
class eq_recorder : public channel_equalizer
{
  std::unique_ptr<channel_equalizer> inner;
  eq_call&                           last;

public:
  eq_recorder(std::unique_ptr<channel_equalizer> inner_, eq_call& last_) : inner(std::move(inner_)), last(last_) {}
  void equalize(span<cf_t> eq_symbols, span<float> eq_noise_vars, const re_buffer_reader<cbf16_t>& ch_symbols, const ch_est_list& ch_estimates,
                span<const float> noise_var_estimates, float tx_scaling) override
  {
    if (tx_scaling != 1.0F) {
      std::fprintf(stderr, "equaliser: scaling %g\n", tx_scaling);
      std::exit(1);
    }
    inner->equalize(eq_symbols, eq_noise_vars, ch_symbols, ch_estimates, noise_var_estimates, tx_scaling);
    last.symbols.assign(eq_symbols.begin(), eq_symbols.end());
    last.noise_vars.assign(eq_noise_vars.begin(), eq_noise_vars.end());
    last.port_noise_vars.assign(noise_var_estimates.begin(), noise_var_estimates.end());
  }
};

struct Cfg {
  int              numerology, slot, bwp_size, bwp_start, prb, nprb, start, ns, rnti, n_id, n_id_0, nack, nsr, ncsi1;
  std::vector<int> ports;
  int              grid_ports, grid_prb;
  int              A() const { return nack + nsr + ncsi1; }
  int              first_prb() const { return bwp_start + prb; }
};
enum Kind { SENT, ZERO, NOISE_ONLY };
struct Entry {
  Cfg  cfg;
  bool sent;
  int  source;
};
struct Group {
  int                group;
  Kind               kind;
  std::vector<Entry> entries; // where kind is SENT, the first one's UE is sent
  double             sigma;   // noise-only: per component
};

// make_cfg of tests/pucch2_model.py: the fields an entry lacks.
Cfg defaults()
{
  return {0, 0, 275, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, {0}, 1, 275};
}

// The ten SHAPES of tests/test_pucch_format2.py on its grid of 4 ports x 52 PRB (bwp_size = 52 - bwp_start), then two more.
// {numerology, slot, bwp_size, bwp_start, starting_prb, nof_prb, start symbol, symbols, rnti, n_id, n_id_0, HARQ-ACK, SR, CSI part 1}, ports.
std::vector<Cfg> small_shapes()
{
  return {
      {0, 3, 49, 3, 48, 1, 13, 1, 4660, 77, 1001, 3, 0, 0, {2}, 4, 52},               // 1 PRB, 1 symbol, 1 port, A 3, last PRB of a BWP from 3
      {1, 19, 52, 0, 7, 1, 12, 2, 65535, 1023, 65535, 2, 1, 9, {3, 1}, 4, 52},        // 1 PRB, 2 symbols, 2 ports, A 12, 64-bit seed
      {0, 9, 52, 0, 20, 2, 13, 1, 17, 5, 9, 4, 0, 7, {2, 0, 3}, 4, 52},               // 2 PRB, 1 symbol, 3 ports, A 11
      {0, 5, 42, 10, 40, 2, 12, 2, 999, 300, 40000, 8, 2, 10, {3, 1, 0, 2}, 4, 52},   // 2 PRB, 2 symbols, 4 ports, A 20, BWP from 10
      {0, 0, 52, 0, 0, 3, 5, 1, 2, 1, 3, 0, 0, 19, {0, 1, 2, 3}, 4, 52},              // 3 PRB, 1 symbol, 4 ports, A 19
      {1, 7, 52, 0, 30, 3, 12, 2, 40000, 512, 123, 20, 0, 0, {1, 2}, 4, 52},          // 3 PRB, 2 symbols, 2 ports, A 20, numerology 1
      {0, 1, 52, 0, 5, 16, 13, 1, 321, 11, 22, 12, 0, 0, {1, 0, 3, 2}, 4, 52},        // 16 PRB, 1 symbol, 4 ports, A 12
      {0, 8, 48, 4, 32, 16, 12, 2, 12345, 678, 54321, 200, 4, 194, {2, 3, 0, 1}, 4, 52}, // 16 PRB, 2 symbols, 4 ports, A 398, BWP from 4
      {0, 2, 52, 0, 51, 1, 0, 2, 7, 8, 9, 19, 0, 0, {0}, 4, 52},                      // 1 PRB, 2 symbols, 1 port, A 19
      {0, 6, 52, 0, 13, 1, 13, 1, 100, 200, 300, 11, 0, 0, {0, 2, 1, 3}, 4, 52},      // 1 PRB, 1 symbol, 4 ports, A 11
      {0, 4, 52, 0, 36, 16, 6, 1, 2001, 45, 4097, 40, 0, 60, {1}, 4, 52},             // 16 PRB, 1 symbol, 1 port, A 100
      {0, 7, 52, 0, 25, 2, 3, 2, 555, 901, 777, 7, 0, 0, {3}, 4, 52},                 // 2 PRB, 2 symbols, 1 port, A 7
  };
}

// The end of the band around the threshold T that no recorded short-block metric lies in: 2 T, but on 1 PRB x 1 symbol.  The
// metric is 31 m^2 / (32 n - m^2), m the best correlation and n the squared norm of the 32 dematched soft bits; of E < 32 soft bits
// m^2 <= E n, so the metric cannot exceed 31 E / (32 - E) -- 31 for E = 16, below 2 T from A = 5 on.  There the band ends half way
// between T and that bound.
double band_end(double T, unsigned E)
{
  return E < 32 ? std::min(2 * T, (T + 31.0 * E / (32.0 - E)) / 2) : 2 * T;
}

double opt(const std::optional<float>& v) { return v.has_value() ? (double)v.value() : NaN; }

struct Result {
  double                row[COLS];
  std::vector<cf_t>     pilots;   // [P][4 nprb]
  std::vector<uint32_t> estimate; // [P][ns][12 nprb]
  std::vector<float>    eq;       // [8 nprb ns][3]
  std::vector<int8_t>   llr;
  std::vector<uint8_t>  decoded;
  bool                  fragile;
  std::string           why; // what made the draw fragile, for the message when every draw is
};

struct Reference {
  std::vector<std::vector<cf_t>>                     smoothed;
  std::vector<ta_call>                               ta_log;
  eq_call                                            eq_last;
  std::unique_ptr<dmrs_pucch_processor_format2_impl> estimator;
  std::unique_ptr<pucch_demodulator_impl>            demodulator;
  std::unique_ptr<uci_decoder_impl>                  decoder;
  channel_estimate                                   estimates;
  pseudo_random_generator_impl                       prg;
  short_block_encoder_impl                           short_encoder;
  polar_code_impl                                    code;
  polar_allocator_impl                               allocator;
  polar_encoder_impl                                 encoder;
  polar_rate_matcher_impl                            rate_matcher;
  crc_calculator_generic_impl                        crc6, crc11;

  Reference() : crc6(crc_generator_poly::CRC6), crc11(crc_generator_poly::CRC11)
  {
    dft_processor::configuration dft_cfg;
    dft_cfg.size = DFT;
    dft_cfg.dir  = dft_processor::direction::INVERSE;
    estimator    = std::make_unique<dmrs_pucch_processor_format2_impl>(
        std::make_unique<pseudo_random_generator_impl>(),
        std::make_unique<port_channel_estimator_average_impl>(
            std::make_unique<interpolator_recorder>(std::make_unique<interpolator_linear_impl>(), smoothed),
            std::make_unique<ta_recorder>(
                std::make_unique<time_alignment_estimator_dft_impl>(std::make_unique<dft_processor_generic_impl>(dft_cfg)), ta_log),
            port_channel_estimator_fd_smoothing_strategy::filter,
            /*compensate_cfo =*/true));
    demodulator = std::make_unique<pucch_demodulator_impl>(
        std::make_unique<eq_recorder>(std::make_unique<channel_equalizer_generic_impl>(channel_equalizer_algorithm_type::zf), eq_last),
        std::make_unique<demodulation_mapper_impl>(),
        std::make_unique<pseudo_random_generator_impl>());
    decoder = std::make_unique<uci_decoder_impl>(std::make_unique<short_block_detector_impl>(),
                                                 std::make_unique<polar_code_impl>(),
                                                 std::make_unique<polar_rate_dematcher_impl>(),
                                                 std::make_unique<polar_decoder_impl>(std::make_unique<polar_encoder_impl>(), 10),
                                                 std::make_unique<polar_deallocator_impl>(),
                                                 std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC6),
                                                 std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC11));
  }

  // The codeword of a message in E bits, as record_uci_reference.cpp makes it.
  std::vector<uint8_t> encode(const std::vector<uint8_t>& msg, unsigned E)
  {
    const unsigned       A = msg.size();
    std::vector<uint8_t> cw(E, 0);
    if (A <= 11) {
      short_encoder.encode(cw, msg, modulation_scheme::QPSK);
      return cw;
    }
    const unsigned  C = get_nof_uci_codeblocks(A, E), L = get_uci_crc_size(A), Eb = E / C;
    crc_calculator& crc = L == 11 ? (crc_calculator&)crc11 : (crc_calculator&)crc6;
    unsigned        first = 0;
    for (unsigned r = 0; r != C; ++r) {
      const unsigned       filler = r == 0 ? A % C : 0, len = r == 0 ? A / C : (A + C - 1) / C;
      std::vector<uint8_t> block(filler, 0);
      block.insert(block.end(), msg.begin() + first, msg.begin() + first + len);
      first += len;
      const crc_calculator_checksum_t checksum = crc.calculate_bit(block);
      for (unsigned b = 0; b != L; ++b) {
        block.push_back((uint8_t)((checksum >> (L - 1 - b)) & 1U));
      }
      code.set(block.size(), Eb, 10, polar_code_ibil::present);
      std::vector<uint8_t> u(code.get_N()), d(code.get_N());
      allocator.allocate(u, block, code);
      encoder.encode(d, u, code.get_n());
      rate_matcher.rate_match(span<uint8_t>(cw).subspan(r * Eb, Eb), d, code);
    }
    return cw;
  }

  // What the UE of `c` sends: x[symbol offset][12 nprb], unit power.
  std::vector<std::vector<cd>> transmit(const Cfg& c, const std::vector<uint8_t>& msg)
  {
    const unsigned       E = 16 * c.nprb * c.ns;
    std::vector<uint8_t> cw = encode(msg, E), b(E);
    prg.init((unsigned)c.rnti * 32768U + (unsigned)c.n_id);
    prg.apply_xor(span<uint8_t>(b), span<const uint8_t>(cw));
    std::vector<std::vector<cd>> x(c.ns, std::vector<cd>(12 * c.nprb));
    unsigned                     at = 0;
    for (int off = 0; off != c.ns; ++off) {
      const uint64_t l = c.start + off, n_id = c.n_id_0;
      const unsigned c_init = (unsigned)((((uint64_t)(14 * c.slot) + l + 1) * (2 * n_id + 1) * 131072ULL + 2 * n_id) & 0x7FFFFFFFULL);
      std::vector<cf_t> r(4 * (c.first_prb() + c.nprb)); // r_l(m) from subcarrier 0 of the grid
      prg.init(c_init);
      static_cast<pseudo_random_generator&>(prg).generate(span<cf_t>(r), (float)M_SQRT1_2);
      for (int k = 0; k != 12 * c.nprb; ++k) {
        if (k % 3 == 1) {
          const cf_t v = r[4 * c.first_prb() + k / 3];
          x[off][k]    = cd(v.real(), v.imag());
        } else {
          x[off][k] = cd(1 - 2 * b[at], 1 - 2 * b[at + 1]) / std::sqrt(2.0);
          at += 2;
        }
      }
    }
    if (at != E) {
      std::fprintf(stderr, "transmitter: %u of %u bits mapped\n", at, E);
      std::exit(1);
    }
    return x;
  }

  // The short-block metric in double from the soft bits, and the message of the best codeword.
  double short_metric(const std::vector<log_likelihood_ratio>& llr, unsigned A, std::vector<uint8_t>& best_msg)
  {
    std::vector<log_likelihood_ratio> tmp(32, log_likelihood_ratio(0));
    for (size_t i = 0; i != llr.size(); ++i) {
      tmp[i % 32] += llr[i];
    }
    double norm = 0.0, best = -1.0;
    for (const log_likelihood_ratio& v : tmp) {
      norm += (double)v.to_int() * v.to_int();
    }
    std::vector<uint8_t> msg(A), cw(32);
    for (unsigned m = 0; m != (1U << A); ++m) {
      for (unsigned i = 0; i != A; ++i) {
        msg[i] = (m >> i) & 1U;
      }
      short_encoder.encode(cw, msg, modulation_scheme::QPSK);
      double dot = 0.0;
      for (unsigned i = 0; i != 32; ++i) {
        dot += (cw[i] ? -1.0 : 1.0) * tmp[i].to_int();
      }
      if (dot > best) {
        best     = dot;
        best_msg = msg;
      }
    }
    return 31.0 * best * best / (32.0 * norm - best * best);
  }

  Result run(word_grid& grid, const Cfg& c, Kind kind, int ig)
  {
    const unsigned P = c.ports.size(), N = 4 * c.nprb, E = 16 * c.nprb * c.ns;
    const double   scs = 15000.0 * (1 << c.numerology);
    grid.map.assign(c.ports.begin(), c.ports.end());
    grid.map.resize(grid.ports, 0);

    dmrs_pucch_processor::config_t e;
    e.format               = pucch_format::FORMAT_2;
    e.slot                 = slot_point(c.numerology, 0, c.slot);
    e.cp                   = cyclic_prefix::NORMAL;
    e.group_hopping        = pucch_group_hopping::NEITHER;
    e.start_symbol_index   = c.start;
    e.nof_symbols          = c.ns;
    e.starting_prb         = c.bwp_start + c.prb;
    e.intra_slot_hopping   = false;
    e.second_hop_prb       = 0;
    e.nof_prb              = c.nprb;
    e.initial_cyclic_shift = 0;
    e.time_domain_occ      = 0;
    e.additional_dmrs      = false;
    e.n_id                 = c.n_id;
    e.n_id_0               = c.n_id_0;
    for (unsigned i = 0; i != P; ++i) {
      e.ports.push_back((uint8_t)i);
    }
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
    smoothed.clear();
    ta_log.clear();
    estimator->estimate(estimates, grid, e);
    channel_state_information csi;
    estimates.get_channel_state_information(csi);

    std::vector<log_likelihood_ratio>        llr(E);
    pucch_demodulator::format2_configuration d;
    for (unsigned i = 0; i != P; ++i) {
      d.rx_ports.push_back((uint8_t)i);
    }
    d.first_prb          = c.bwp_start + c.prb;
    d.nof_prb            = c.nprb;
    d.start_symbol_index = c.start;
    d.nof_symbols        = c.ns;
    d.rnti               = c.rnti;
    d.n_id               = c.n_id;
    demodulator->demodulate(llr, grid, estimates, d);

    Result r;
    r.fragile = false;
    r.decoded.assign(c.A(), 0);
    uci_decoder::configuration dec;
    dec.modulation          = modulation_scheme::QPSK;
    const uci_status status = decoder->decode(r.decoded, llr, dec);
    for (const log_likelihood_ratio& v : llr) {
      r.llr.push_back(v.to_value_type());
    }
    for (double& v : r.row) {
      v = NaN;
    }
    r.row[0] = status == uci_status::valid ? 1 : (status == uci_status::invalid ? 2 : 0);
    const bool silent = std::all_of(r.llr.begin(), r.llr.end(), [](int8_t v) { return v == 0; });
    if (c.A() <= 11 && !silent) {
      std::vector<uint8_t> best_msg;
      r.row[1] = short_metric(llr, c.A(), best_msg);
      const double T = THRESHOLDS[c.A() - 1];
      r.fragile  = r.row[1] >= T / 2 && r.row[1] <= band_end(T, E);
      r.why += r.fragile ? " short-block metric" : "";
      if (!r.fragile && (best_msg != r.decoded || (r.row[1] > T) != (status == uci_status::valid))) {
        std::fprintf(stderr, "group %d: the short-block metric in double, %g, is not what the reference decided on\n", ig, r.row[1]);
        std::exit(1);
      }
    }
    r.row[2] = opt(csi.get_sinr_dB());
    r.row[3] = opt(csi.get_rsrp_dB());
    r.row[4] = opt(csi.get_epre_dB());
    r.row[5] = csi.get_time_alignment().has_value() ? csi.get_time_alignment().value().to_seconds() : NaN;
    r.row[6] = opt(csi.get_cfo_Hz());

    if (smoothed.size() != P || ta_log.size() != P) {
      std::fprintf(stderr, "group %d: %zu interpolations and %zu time alignments for %u ports\n", ig, smoothed.size(), ta_log.size(), P);
      std::exit(1);
    }
    if (eq_last.symbols.size() != 8U * c.nprb * c.ns || eq_last.noise_vars.size() != eq_last.symbols.size() || eq_last.port_noise_vars.size() != P) {
      std::fprintf(stderr, "group %d: %zu equalised symbols, %u expected\n", ig, eq_last.symbols.size(), 8U * c.nprb * c.ns);
      std::exit(1);
    }
    for (size_t i = 0; i != eq_last.symbols.size(); ++i) {
      r.eq.push_back(eq_last.symbols[i].real());
      r.eq.push_back(eq_last.symbols[i].imag());
      r.eq.push_back(eq_last.noise_vars[i]);
    }
    std::vector<double> k(N); // the pilots' grid subcarriers
    double              mean = 0.0, var = 0.0;
    for (unsigned q = 0; q != N; ++q) {
      k[q] = 12 * c.first_prb() + 3 * q + 1;
      mean += k[q] / N;
    }
    for (unsigned q = 0; q != N; ++q) {
      var += (k[q] - mean) * (k[q] - mean) / N;
    }
    const double asked = std::min(MARGIN, 0.5 * (2 * M_PI / DFT) * (2 * M_PI / DFT) * var);
    double       snr[2] = {0.0, 0.0};
    unsigned     best_port = 0;
    for (unsigned p = 0; p != P; ++p) {
      const std::vector<cf_t>& f  = smoothed[p];
      const ta_call&           ta = ta_log[p];
      bool                     same = f.size() == N && ta.symbols.size() == N && ta.subc.size() == N && ta.scs_khz * 1000.0 == scs;
      for (unsigned q = 0; same && q != N; ++q) {
        same = std::memcmp(&f[q], &ta.symbols[q], sizeof(cf_t)) == 0 && ta.subc[q] == (unsigned)k[q];
      }
      if (!same) {
        std::fprintf(stderr, "group %d: the time alignment estimator was not handed the smoothed pilots\n", ig);
        std::exit(1);
      }
      if (eq_last.port_noise_vars[p] != estimates.get_noise_variance(p)) {
        std::fprintf(stderr, "group %d: the equaliser was not handed port %u's noise variance\n", ig, p);
        std::exit(1);
      }
      double best = -1.0, second = -1.0;
      int    best_bin = 0;
      for (int b = -TA_WINDOW; b != TA_WINDOW; ++b) {
        cd x = 0.0;
        for (unsigned q = 0; q != N; ++q) {
          x += cd(f[q].real(), f[q].imag()) * std::polar(1.0, 2 * M_PI * (double)b * k[q] / DFT);
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
      const bool   near = best - second < asked * best;
      const double bin  = ta.answer * DFT * scs;
      if (kind == SENT) {
        r.fragile = r.fragile || near;
        r.why += near ? " time alignment lead" : "";
        if (!near && (std::fabs(bin - std::round(bin)) > 1e-6 || (int)std::round(bin) != best_bin)) {
          std::fprintf(stderr, "group %d port %u: the reference's bin %g, %d in double with a lead of %g\n", ig, p, bin, best_bin, (best - second) / best);
          std::exit(1);
        }
      }
      double* o = r.row + 8 + 10 * p;
      o[0]      = estimates.get_noise_variance(p);
      o[1]      = estimates.get_rsrp(p);
      o[2]      = estimates.get_epre(p);
      o[3]      = estimates.get_snr(p);
      o[4]      = opt(estimates.get_cfo_Hz(p));
      o[5]      = ta.answer;
      o[6]      = std::round(bin);
      o[7]      = best;
      o[8]      = second;
      o[9]      = asked;
      if (o[3] > snr[0]) {
        snr[1]    = snr[0];
        snr[0]    = o[3];
        best_port = p;
      } else if (o[3] > snr[1]) {
        snr[1] = o[3];
      }
      r.pilots.insert(r.pilots.end(), f.begin(), f.end());
    }
    r.row[7] = best_port;
    if (kind != ZERO && P > 1) {
      r.fragile = r.fragile || (snr[0] - snr[1] < MARGIN * snr[0]);
      r.why += snr[0] - snr[1] < MARGIN * snr[0] ? " best port" : "";
    }
    // The estimate: the region in [P][symbol][subcarrier] order, nothing else written (but for the rotated mark).
    const uint32_t same = word_of(untouched);
    const unsigned k0 = 12 * c.first_prb(), k1 = k0 + 12 * c.nprb;
    for (unsigned p = 0; p != P; ++p) {
      for (int l = 0; l != 14; ++l) {
        span<const cbf16_t> row    = estimates.get_symbol_ch_estimate(l, p);
        const bool          inside = l >= c.start && l < c.start + c.ns;
        uint32_t            mark   = same;
        for (unsigned q = 0; q != row.size(); ++q) {
          if (!(inside && q >= k0 && q < k1)) {
            mark = word_of(row[q]);
            break;
          }
        }
        const cf_t m = cf_t(bf16_value(mark & 0xFFFFU), bf16_value(mark >> 16));
        if (mark != same && !(inside && c.ns == 2 && std::fabs(std::abs(m) - std::sqrt(98.0F)) < 0.05F)) {
          std::fprintf(stderr, "group %d: port %u symbol %d was written outside the allocation\n", ig, p, l);
          std::exit(1);
        }
        for (unsigned q = 0; q != row.size(); ++q) {
          if (inside && q >= k0 && q < k1) {
            r.estimate.push_back(word_of(row[q]));
          } else if (word_of(row[q]) != mark) {
            std::fprintf(stderr, "group %d: port %u symbol %d subcarrier %u was written\n", ig, p, l, q);
            std::exit(1);
          }
        }
      }
    }
    return r;
  }
};

std::string floats_json(const std::vector<double>& v)
{
  std::string s = "[";
  for (size_t i = 0; i != v.size(); ++i) {
    char num[40];
    std::snprintf(num, sizeof(num), "%.17g", v[i]);
    s += (i ? ", " : "") + std::string(num);
  }
  return s + "]";
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s pf2_configs.json OUT\n", argv[0]);
    return 1;
  }
  std::ifstream     in(argv[1]);
  std::stringstream buffer;
  buffer << in.rdbuf();
  const std::string text = buffer.str();
  const std::string dir  = argv[2];

  // Group 0: fixture_cfgs() of the test file, restated.  The file's objects are flat and come in the order processor, demodulator,
  // dmrs; the validator's objects have neither a grid nor a hopping flag.
  std::vector<Group> groups;
  {
    const std::regex object("\\{[^{}]*\\}");
    int              source = 0;
    for (std::sregex_iterator it(text.begin(), text.end(), object), end; it != end; ++it) {
      const std::string o = it->str();
      Cfg               c = defaults();
      if (o.find("\"first_prb\"") != std::string::npos) {
        c.prb      = json_int(o, "first_prb");
        c.bwp_size = json_int(o, "grid_nof_prb");
        c.grid_prb = c.bwp_size;
        c.nack     = 4;
      } else if (o.find("\"intra_slot_hopping\"") != std::string::npos) {
        if (json_int(o, "intra_slot_hopping", 0)) {
          continue;
        }
        c.prb  = json_int(o, "starting_prb");
        c.nack = 4;
      } else if (o.find("\"grid_nof_prb\"") != std::string::npos) {
        c.prb       = json_int(o, "starting_prb");
        c.bwp_size  = json_int(o, "bwp_size_rb");
        c.bwp_start = json_int(o, "bwp_start_rb");
        c.grid_prb  = json_int(o, "grid_nof_prb");
        c.nack      = json_int(o, "nof_harq_ack");
        c.nsr       = json_int(o, "nof_sr");
        c.ncsi1     = json_int(o, "nof_csi_part1");
        if (json_int(o, "nof_csi_part2") != 0) {
          std::fprintf(stderr, "configuration %d has CSI part 2\n", source);
          return 1;
        }
      } else {
        continue;
      }
      c.numerology = json_int(o, "numerology", c.numerology);
      c.slot       = json_int(o, "slot_index", c.slot);
      c.nprb       = json_int(o, "nof_prb");
      c.start      = json_int(o, "start_symbol_index");
      c.ns         = json_int(o, "nof_symbols");
      c.rnti       = json_int(o, "rnti", c.rnti);
      c.n_id       = json_int(o, "n_id", c.n_id);
      c.n_id_0     = json_int(o, "n_id_0", c.n_id_0);
      c.ports      = json_list(o, "rx_ports");
      c.grid_ports = *std::max_element(c.ports.begin(), c.ports.end()) + 1;
      groups.push_back({0, SENT, {{c, true, source++}}, 0.0});
    }
  }
  const size_t nof_fixture = groups.size();
  const std::vector<Cfg> shapes = small_shapes();
  for (size_t i = 0; i != shapes.size(); ++i) {
    groups.push_back({1, SENT, {{shapes[i], true, (int)i}}, 0.0});
  }
  {
    Cfg a = shapes[3], b = shapes[3]; // 2 PRB, 2 symbols, 4 ports
    a.nack = 3, a.nsr = 0, a.ncsi1 = 0;
    b.nack = 12, b.nsr = 0, b.ncsi1 = 0;
    groups.push_back({2, ZERO, {{a, false, 0}, {b, false, 1}}, 0.0});
  }
  for (int k = 0; k != 16; ++k) { // noise only
    // ports 1, 2, 4; PRBs 1, 2, 3, 16; symbols 1, 2; A <= 11 for even k.  One symbol admits A >= 12 from 2 PRB on.
    static const int widths[4] = {1, 2, 3, 16}, short_sizes[4] = {3, 11, 7, 5};
    const int        nprb = widths[(k / 2) % 4], ns = (k % 2 && nprb == 1) ? 2 : 1 + (k / 8 + k / 2) % 2;
    const int        A    = k % 2 ? (nprb == 16 ? 40 : 12) : short_sizes[(k / 4) % 4];
    std::vector<int> ports = k % 3 == 0 ? std::vector<int>{1} : k % 3 == 1 ? std::vector<int>{2, 0} : std::vector<int>{0, 1, 2, 3};
    Cfg              c = {k % 2, (1 + k) % 10, 52, 0, (5 * k) % (53 - nprb), nprb, 14 - ns - (k % 5), ns, 1000 + 77 * k, 10 + 60 * k,
                          500 + 4000 * k, A, 0, 0, ports, 4, 52};
    groups.push_back({3, NOISE_ONLY, {{c, false, k}}, std::pow(10.0, -3.0 + 4.0 * k / 15.0)});
  }
  {
    int source = 0;
    for (int i : {1, 5, 7}) { // A 12 (parity-check bits), A 20 (CRC11) and A 398
      Group g = {4, SENT, {{shapes[i], true, source++}}, 0.0};
      Cfg   o = shapes[i];
      o.rnti ^= 1;
      g.entries.push_back({o, false, source++});
      o = shapes[i];
      o.n_id ^= 1;
      g.entries.push_back({o, false, source++});
      o = shapes[i];
      o.n_id_0 ^= 1;
      g.entries.push_back({o, false, source++});
      groups.push_back(g);
    }
  }

  Reference                              ref;
  std::mt19937                           rng(20261021);
  std::normal_distribution<double>       normal(0.0, 1.0);
  std::uniform_real_distribution<double> uniform(0.0, 1.0);
  std::vector<uint32_t>                  grids, estimates;
  std::vector<cf_t>                      pilots;
  std::vector<float>                     eqs;
  std::vector<int8_t>                    llrs;
  std::vector<uint8_t>                   messages;
  std::vector<double>                    results;
  std::ostringstream                     json;
  size_t                                 nof_cases = 0, draws_total = 0;
  json << "[\n";
  for (size_t ig = 0; ig != groups.size(); ++ig) {
    const Group& g = groups[ig];
    const Cfg&   c = g.entries[0].cfg;
    for (const Entry& e : g.entries) { // one region per group
      const Cfg& o = e.cfg;
      if (o.ports != c.ports || o.start != c.start || o.ns != c.ns || o.first_prb() != c.first_prb() || o.nprb != c.nprb ||
          o.numerology != c.numerology || o.grid_prb != c.grid_prb || o.grid_ports != c.grid_ports || o.grid_prb < o.bwp_start + o.bwp_size) {
        std::fprintf(stderr, "group %zu: its cases do not share a region\n", ig);
        return 1;
      }
    }
    const unsigned            P  = c.ports.size();
    const std::vector<double> ep = epochs(c.numerology);
    word_grid                 grid(c.grid_ports, 12 * c.grid_prb);
    std::vector<Result>       res;
    std::string               why;
    std::vector<uint8_t>      msg(c.A());
    std::vector<double>       snr_db(P, 0.0);
    double                    d0 = 0.0, d1 = 0.0, cfo = 0.0, sigma = 0.0;
    unsigned                  draws = 0;
    bool                      fragile;
    for (uint8_t& b : msg) {
      b = (uint8_t)(rng() & 1U);
    }
    std::vector<std::vector<cd>> x;
    if (g.kind == SENT) {
      x = ref.transmit(c, msg);
    }
    do {
      ++draws;
      std::vector<cd> g0(P, 0.0), g1(P, 0.0);
      if (g.kind == SENT) {
        d0  = 8 * uniform(rng);
        d1  = d0 + 5 + 25 * uniform(rng);
        cfo = 0.02 * uniform(rng) - 0.01;
        for (unsigned p = 0; p != P; ++p) {
          snr_db[p]        = 16.0 + 8 * uniform(rng);
          const double amp = std::pow(10.0, snr_db[p] / 20);
          cd           a   = amp * cd(normal(rng), normal(rng)) / std::sqrt(2.0);
          if (std::abs(a) < 0.5 * amp) {
            a = std::polar(0.5 * amp, std::arg(a));
          }
          g0[p] = a;
          g1[p] = 0.3 * amp * cd(normal(rng), normal(rng)) / std::sqrt(2.0);
        }
      }
      sigma = g.kind == SENT ? std::sqrt(0.5) : g.kind == NOISE_ONLY ? g.sigma : 0.0;
      for (unsigned p = 0; p != P; ++p) {
        for (int off = 0; off != c.ns; ++off) {
          const cd rot = std::polar(1.0, 2 * M_PI * cfo * ep[c.start + off]);
          for (int n = 0; n != 12 * c.nprb; ++n) {
            const double k = 12 * c.first_prb() + n;
            cd           v = sigma * cd(normal(rng), normal(rng));
            if (g.kind == SENT) {
              v += (g0[p] * std::polar(1.0, -2 * M_PI * k * d0 / DFT) + g1[p] * std::polar(1.0, -2 * M_PI * k * d1 / DFT)) * rot * x[off][n];
            }
            grid.set(c.ports[p], c.start + off, (unsigned)k, (float)v.real(), (float)v.imag());
          }
        }
      }
      res.clear();
      why.clear();
      fragile = false;
      for (const Entry& e : g.entries) {
        res.push_back(ref.run(grid, e.cfg, g.kind, (int)ig));
        const Result& r = res.back();
        fragile         = fragile || (g.kind != ZERO && r.fragile);
        if (e.sent) {
          fragile = fragile || r.row[0] != 1 || r.decoded != msg;
          why     = r.row[0] != 1 || r.decoded != msg ? " message not returned" : "";
        }
        why += r.why;
      }
    } while (fragile && draws != 10000);
    if (fragile) {
      std::fprintf(stderr, "group %zu: every draw fragile, the last one by%s\n", ig, why.c_str());
      return 1;
    }
    draws_total += draws;
    const size_t grid_off = grids.size();
    for (unsigned p = 0; p != P; ++p) {
      for (int off = 0; off != c.ns; ++off) {
        for (int n = 0; n != 12 * c.nprb; ++n) {
          grids.push_back(grid.word(c.ports[p], c.start + off, 12 * c.first_prb() + n));
        }
      }
    }
    for (size_t ie = 0; ie != g.entries.size(); ++ie) {
      const Entry&  e = g.entries[ie];
      const Cfg&    o = e.cfg;
      const Result& r = res[ie];
      json << (nof_cases ? ",\n" : "") << "{\"numerology\": " << o.numerology << ", \"slot_index\": " << o.slot << ", \"bwp_size_rb\": " << o.bwp_size
           << ", \"bwp_start_rb\": " << o.bwp_start << ", \"starting_prb\": " << o.prb << ", \"nof_prb\": " << o.nprb
           << ", \"start_symbol_index\": " << o.start << ", \"nof_symbols\": " << o.ns << ", \"rnti\": " << o.rnti << ", \"n_id\": " << o.n_id
           << ", \"n_id_0\": " << o.n_id_0 << ", \"nof_harq_ack\": " << o.nack << ", \"nof_sr\": " << o.nsr << ", \"nof_csi_part1\": " << o.ncsi1
           << ", \"nof_csi_part2\": 0, \"rx_ports\": " << list_json(o.ports) << ", \"grid_nof_ports\": " << o.grid_ports
           << ", \"grid_nof_prb\": " << o.grid_prb << ", \"group\": " << g.group << ", \"source\": " << e.source
           << ", \"flags\": " << (g.kind == ZERO ? 1 : 0) << ", \"draws\": " << draws << ", \"A\": " << o.A() << ", \"sent\": " << (e.sent ? 1 : 0)
           << ", \"snr_db\": " << floats_json(snr_db) << ", \"delay\": " << floats_json({d0}) << ", \"delay2\": " << floats_json({d1})
           << ", \"cfo\": " << floats_json({cfo}) << ", \"sigma\": " << floats_json({sigma}) << ", \"grid_off\": " << grid_off
           << ", \"pilot_off\": " << pilots.size() << ", \"est_off\": " << estimates.size() << ", \"eq_off\": " << eqs.size() / 3
           << ", \"llr_off\": " << llrs.size() << ", \"msg_off\": " << messages.size() << ", \"res_row\": " << nof_cases << "}";
      pilots.insert(pilots.end(), r.pilots.begin(), r.pilots.end());
      estimates.insert(estimates.end(), r.estimate.begin(), r.estimate.end());
      eqs.insert(eqs.end(), r.eq.begin(), r.eq.end());
      llrs.insert(llrs.end(), r.llr.begin(), r.llr.end());
      if (e.sent) {
        messages.insert(messages.end(), msg.begin(), msg.end());
      }
      messages.insert(messages.end(), r.decoded.begin(), r.decoded.end());
      results.insert(results.end(), r.row, r.row + COLS);
      ++nof_cases;
    }
  }
  json << "\n]\n";
  std::ofstream(dir + "/pf2_reference_cases.json") << json.str();
  write_npy(dir + "/pf2_reference_grids.npy", "<u4", grids, 0);
  write_npy(dir + "/pf2_reference_pilots.npy", "<c8", pilots, 0);
  write_npy(dir + "/pf2_reference_estimates.npy", "<u4", estimates, 0);
  write_npy(dir + "/pf2_reference_eq.npy", "<f4", eqs, 3);
  write_npy(dir + "/pf2_reference_llr.npy", "|i1", llrs, 0);
  write_npy(dir + "/pf2_reference_messages.npy", "|u1", messages, 0);
  write_npy(dir + "/pf2_reference_results.npy", "<f8", results, COLS);
  std::printf("%zu cases (%zu of the reference's) in %zu grids, %zu draws; %zu grid words, %zu pilots, %zu estimate words, %zu equalised "
              "symbols, %zu soft bits, %zu message bytes\n",
              nof_cases, nof_fixture, groups.size(), draws_total, grids.size(), pilots.size(), estimates.size(), eqs.size() / 3, llrs.size(),
              messages.size());
  return 0;
}
