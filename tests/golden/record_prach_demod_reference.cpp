// Records the answers of srsRAN-5G-ER's ofdm_prach_demodulator_impl for tests/test_prach_demodulator.py.  It constructs the
// reference's classes directly (dft_processor_generic_impl, prach_buffer_impl), feeds them seeded inputs and writes the outputs as
// .npy files; it also prints the reference's preamble, window and frequency mapping tables.  Built and run by
// oracle/recorders.mk, against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`,
// `make -C oracle rerecord-check`; no binary or object is committed.
//
//   record_prach_demod_reference prach_demod_configs.json OUT       the recording
//   record_prach_demod_reference --tables > prach_demod_tables.json the tables
//
// The cases are the entries of prach_demod_configs.json followed by EXTRA below (what the unit test's header leaves out).
// Inputs are not stored.  Sample n of case c has real part value(2 n) and imaginary part value(2 n + 1) of the sequence
//   x <- x * 6364136223846793005 + 1442695040888963407 (mod 2^64), starting from x = (c + 1) * 0x9E3779B97F4A7C15 (mod 2^64),
//   value = ((x >> 40) - 2^23) / 2^23 after each step: 24 bits, exact in float32.
// Files (case i is row i of `cases`):
//   prach_demod_reference_cases.npy  int64 [n][12]: sampling rate in Hz, format (0, 1, 2, 3, A1, A2, A3, B1, B4, C0, C2, A1/B1,
//                                    A2/B2, A3/B3 as 0..13), td occasions, fd occasions, start symbol, RB offset, grid PRB, PUSCH
//                                    numerology, input samples, output file, offset into it, output elements
//   prach_demod_reference_out<k>.npy complex64, the buffers of the cases back to back, each as [td][fd][symbol][L_RA]; a file
//                                    holds whole cases and stays below 900000 bytes
#include "lib/phy/generic_functions/dft_processor_generic_impl.h"
#include "lib/phy/lower/modulation/ofdm_prach_demodulator_impl.h"
#include "lib/phy/support/prach_buffer_impl.h"
#include "recorder_io.h"
#include "srsran/ran/prach/prach_frequency_mapping.h"
#include "srsran/ran/prach/prach_preamble_information.h"

#include <complex>

using namespace srsran;

namespace {

const char* FORMATS[14] = {"0", "1", "2", "3", "A1", "A2", "A3", "B1", "B4", "C0", "C2", "A1/B1", "A2/B2", "A3/B3"};

struct Case {
  long srate, format, ntd, nfd, start, rb, nprb, mu;
};

// Ground the header leaves out: a sequence across the grid centre, one above it, 1, 4 and 8 fd occasions, every split transform
// size (9216 ... 49152) and every size one LDS transform takes (256 ... 6144), format 3, short formats at 60 and 120 kHz, a
// start in the middle of the slot with an occasion across 0.5 ms, a mixed format's last occasion.
const Case EXTRA[] = {
    {30720000, 0, 1, 1, 0, 39, 79, 0},   // 24576, across the centre
    {30720000, 0, 1, 4, 0, 45, 79, 0},   // above the centre, 4 fd
    {30720000, 0, 1, 8, 0, 0, 79, 0},    // 8 fd, the seventh across the centre
    {11520000, 0, 1, 2, 0, 2, 25, 0},    // 9216 = 3 x 3072
    {15360000, 0, 1, 2, 0, 2, 52, 0},    // 12288 = 3 x 4096
    {23040000, 0, 1, 2, 0, 30, 79, 0},   // 18432 = 6 x 3072
    {46080000, 0, 1, 1, 0, 3, 106, 1},   // 36864 = 12 x 3072, K = 24
    {61440000, 0, 1, 3, 0, 90, 160, 1},  // 49152 = 12 x 4096, above the centre
    {46080000, 3, 1, 2, 0, 10, 51, 1},   // format 3 on 9216, 4 symbols
    {7680000, 0, 1, 2, 0, 1, 25, 0},     // 6144 in one transform
    {7680000, 1, 1, 1, 0, 12, 25, 0},    // 6144, 2 symbols, across the centre
    {30720000, 5, 3, 2, 0, 1, 40, 2},    // A2 at 60 kHz, 512
    {30720000, 8, 1, 1, 0, 2, 20, 3},    // B4 at 120 kHz, 256
    {61440000, 10, 2, 1, 1, 5, 40, 3},   // C2 at 120 kHz, 512
    {30720000, 5, 2, 2, 5, 40, 106, 0},  // A2 from symbol 5: the first occasion crosses 0.5 ms
    {30720000, 13, 2, 2, 2, 60, 106, 0}, // A3/B3 from symbol 2: the last occasion is a B3
    {61440000, 12, 3, 2, 1, 0, 79, 1},   // A2/B2 at 30 kHz from symbol 1
    {23040000, 9, 3, 2, 1, 4, 100, 0},   // C0 on 1536
    {69120000, 7, 2, 1, 0, 200, 275, 0}, // B1 on 4608, above the centre
    {61440000, 6, 1, 3, 7, 100, 270, 0}, // A3 on 4096
    {46080000, 4, 2, 2, 9, 90, 200, 0},  // A1 on 3072
    {15360000, 11, 7, 2, 0, 30, 79, 0},  // A1/B1 on 1024
    {11520000, 4, 3, 1, 3, 20, 52, 0},   // A1 on 768
    {5760000, 4, 2, 1, 6, 9, 25, 0},     // A1 on 384
    {92160000, 8, 1, 4, 2, 110, 275, 0}, // B4 on 6144
    {30720000, 2, 1, 2, 2, 20, 79, 0},   // format 2 from symbol 2
};

unsigned kappa(phy_time_unit t)
{
  return (unsigned)t.to_samples(30720000U); // one kappa is one sample at 30.72 MHz
}

int tables()
{
  std::printf("{\n\"preamble\": [\n");
  bool first = true;
  for (unsigned f = 0; f != 14; ++f) {
    const prach_format_type format = to_prach_format_type(FORMATS[f]);
    for (unsigned mu = 0; mu != (f < 4 ? 1U : 4U); ++mu) {
      for (unsigned last = 0; last != (f < 4 ? 1U : 2U); ++last) {
        const prach_preamble_information info =
            f < 4 ? get_prach_preamble_long_info(format)
                  : get_prach_preamble_short_info(format, static_cast<prach_subcarrier_spacing>(mu), last != 0);
        std::printf("%s{\"format\": \"%s\", \"mu\": %u, \"last\": %u, \"sequence_length\": %u, \"ra_scs\": %u, \"nof_symbols\": %u, "
                    "\"cp_kappa\": %u, \"symbols_kappa\": %u, \"duration\": %u}",
                    first ? "" : ",\n", FORMATS[f], mu, last, info.sequence_length, (unsigned)info.scs, info.nof_symbols,
                    kappa(info.cp_length), kappa(info.symbol_length()), get_preamble_duration(format));
        first = false;
      }
    }
  }
  std::printf("\n],\n\"window\": [\n");
  first = true;
  for (unsigned f = 0; f != 14; ++f) {
    const prach_format_type format = to_prach_format_type(FORMATS[f]);
    const unsigned          dur    = get_preamble_duration(format);
    for (unsigned mu = 0; mu != 4; ++mu) {
      for (unsigned start = 0; start != 14; ++start) {
        for (unsigned ntd = 1; ntd <= (f < 4 ? 1U : 7U); ++ntd) {
          if (f >= 4 && start + dur * ntd > 14) {
            continue;
          }
          std::printf("%s[\"%s\", %u, %u, %u, %u]", first ? "" : ",\n", FORMATS[f], mu, start, ntd,
                      kappa(get_prach_window_duration(format, to_subcarrier_spacing(mu), start, ntd)));
          first = false;
        }
      }
    }
  }
  std::printf("\n],\n\"mapping\": [\n");
  first = true;
  for (unsigned ra = 0; ra != 6; ++ra) {
    for (unsigned mu = 0; mu != 4; ++mu) {
      const prach_frequency_mapping_information m =
          prach_frequency_mapping_get(static_cast<prach_subcarrier_spacing>(ra), to_subcarrier_spacing(mu));
      std::printf("%s[%u, %u, %u, %u]", first ? "" : ",\n", ra, mu, m.nof_rb_ra, m.k_bar);
      first = false;
    }
  }
  std::printf("\n]\n}\n");
  return 0;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc == 2 && std::string(argv[1]) == "--tables") {
    return tables();
  }
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s prach_demod_configs.json OUT | --tables\n", argv[0]);
    return 2;
  }
  std::ifstream     in(argv[1]);
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string text = ss.str();
  const std::regex  entry("\"srate_hz\": (\\d+), \"format\": \"([^\"]+)\", \"nof_td_occasions\": (\\d+), \"nof_fd_occasions\": (\\d+), "
                          "\"start_symbol\": (\\d+), \"rb_offset\": (\\d+), \"nof_prb_ul_grid\": (\\d+), \"pusch_scs_kHz\": (\\d+)");
  std::vector<Case> cases;
  for (std::sregex_iterator it(text.begin(), text.end(), entry), end; it != end; ++it) {
    long f = 0;
    while (f != 14 && (*it)[2] != FORMATS[f]) {
      ++f;
    }
    long mu = 0;
    while ((15L << mu) != std::stol((*it)[8])) {
      ++mu;
    }
    cases.push_back({std::stol((*it)[1]), f, std::stol((*it)[3]), std::stol((*it)[4]), std::stol((*it)[5]), std::stol((*it)[6]),
                     std::stol((*it)[7]), mu});
  }
  std::printf("%zu configurations of the header\n", cases.size());
  cases.insert(cases.end(), std::begin(EXTRA), std::end(EXTRA));

  const std::string                dir = argv[2];
  std::vector<int64_t>             table;
  std::vector<std::complex<float>> shard;
  long                             shard_index = 0;
  auto flush = [&]() {
    write_npy(dir + "/prach_demod_reference_out" + std::to_string(shard_index) + ".npy", "<c8", shard, 0);
    shard.clear();
    ++shard_index;
  };
  for (size_t c = 0; c != cases.size(); ++c) {
    const Case&             k      = cases[c];
    const sampling_rate     srate  = sampling_rate::from_Hz(k.srate);
    const prach_format_type format = to_prach_format_type(FORMATS[k.format]);
    // One transform per spacing whose size the generic DFT has (the demodulator asks only for the occasion's).
    ofdm_prach_demodulator_impl::dft_processors_table dfts;
    static const unsigned SCS_HZ[6] = {15000, 30000, 60000, 120000, 1250, 5000};
    for (unsigned ra = 0; ra != 6; ++ra) {
      dft_processor::configuration cfg = {(unsigned)(k.srate / SCS_HZ[ra]), dft_processor::direction::DIRECT};
      auto                         dft = std::make_unique<dft_processor_generic_impl>(cfg);
      if (dft->is_valid()) {
        dfts.emplace(static_cast<prach_subcarrier_spacing>(ra), std::move(dft));
      }
    }
    ofdm_prach_demodulator_impl demodulator(srate, std::move(dfts));

    const prach_preamble_information info =
        k.format < 4 ? get_prach_preamble_long_info(format)
                     : get_prach_preamble_short_info(format, static_cast<prach_subcarrier_spacing>(k.mu), false);
    const long n_in = get_prach_window_duration(format, to_subcarrier_spacing(k.mu), k.start, k.ntd).to_samples(k.srate);
    std::vector<cf_t> input(n_in);
    uint64_t          x = (uint64_t)(c + 1) * 0x9E3779B97F4A7C15ULL;
    auto              value = [&x]() {
      x = x * 6364136223846793005ULL + 1442695040888963407ULL;
      return (float)((double)((long)(x >> 40) - (1L << 23)) / (double)(1L << 23));
    };
    for (cf_t& v : input) {
      const float re = value();
      const float im = value();
      v              = cf_t(re, im);
    }
    prach_buffer_impl buffer(1, k.ntd, k.nfd, info.nof_symbols, info.sequence_length);
    ofdm_prach_demodulator::configuration config = {format, (unsigned)k.ntd, (unsigned)k.nfd, (unsigned)k.start, (unsigned)k.rb,
                                                    (unsigned)k.nprb, to_subcarrier_spacing(k.mu), 0};
    demodulator.demodulate(buffer, input, config);
    const size_t n_out = (size_t)k.ntd * k.nfd * info.nof_symbols * info.sequence_length;
    if ((shard.size() + n_out) * sizeof(std::complex<float>) > 900000 - 128) {
      flush();
    }
    for (long v : {k.srate, k.format, k.ntd, k.nfd, k.start, k.rb, k.nprb, k.mu, n_in, shard_index, (long)shard.size(), (long)n_out}) {
      table.push_back(v);
    }
    for (unsigned td = 0; td != k.ntd; ++td) {
      for (unsigned fd = 0; fd != k.nfd; ++fd) {
        for (unsigned s = 0; s != info.nof_symbols; ++s) {
          span<const cf_t> sym = const_cast<const prach_buffer_impl&>(buffer).get_symbol(0, td, fd, s);
          shard.insert(shard.end(), sym.begin(), sym.end());
        }
      }
    }
  }
  flush();
  write_npy(dir + "/prach_demod_reference_cases.npy", "<i8", table, 12);
  std::printf("%zu cases in %ld files\n", cases.size(), shard_index);
  return 0;
}
