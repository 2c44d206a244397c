// Records the answers of srsRAN-5G-ER's uci_decoder_impl for tests/test_uci_decoder.py.  It constructs the reference's classes
// directly, feeds them seeded inputs and writes inputs and outputs as four .npy files.  Built and run by oracle/recorders.mk,
// against a checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`, `make -C oracle rerecord-check`; no
// binary or object is committed.
//
// Files (case i is row i of `cases`):
//   uci_reference_cases.npy  int32 [n][8]: message length A, LLR length E, modulation (bits per symbol; 0 = pi/2-BPSK), input kind,
//                            offset into llr, offset into sent / decoded, the reference's uci_status (1 valid, 2 invalid), 0
//   uci_reference_llr.npy    int8, the inputs back to back
//   uci_reference_sent.npy   uint8, the messages that were encoded, one bit per byte
//   uci_reference_decoded.npy uint8, what decode() left in a message buffer that held FILL (2) in every byte before the call
// Input kinds: 0 the codeword at +-20 (the placeholders of 1- and 2-bit messages at 0); 1 and 2 the same plus Gaussian noise of
// standard deviation 8 and 40, rounded and clipped to +-120; 3 all zero; 4 values of +-120 and +-127 with the codeword's signs, one
// in ten flipped.
#include "lib/phy/upper/channel_coding/polar/polar_allocator_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_code_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_deallocator_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_decoder_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_encoder_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_rate_dematcher_impl.h"
#include "lib/phy/upper/channel_coding/polar/polar_rate_matcher_impl.h"
#include "lib/phy/upper/channel_coding/crc_calculator_generic_impl.h"
#include "lib/phy/upper/channel_coding/short/short_block_detector_impl.h"
#include "lib/phy/upper/channel_coding/short/short_block_encoder_impl.h"
#include "lib/phy/upper/channel_processors/uci/uci_decoder_impl.h"
#include "recorder_io.h"
#include "srsran/ran/uci/uci_info.h"

#include <cmath>
#include <random>
#include <set>

using namespace srsran;

namespace {

constexpr uint8_t FILL = 2;

struct Size {
  unsigned A, E, mod; // mod: bits per symbol, 0 = pi/2-BPSK
};

modulation_scheme scheme(unsigned mod)
{
  switch (mod) {
    case 0:
      return modulation_scheme::PI_2_BPSK;
    case 1:
      return modulation_scheme::BPSK;
    case 2:
      return modulation_scheme::QPSK;
    case 4:
      return modulation_scheme::QAM16;
    case 6:
      return modulation_scheme::QAM64;
    default:
      return modulation_scheme::QAM256;
  }
}

// Code length of one block as TS 38.212 Section 5.3.1 gives it (n_max = 10), to keep away from what the reference asserts on.
unsigned code_length(unsigned K, unsigned E)
{
  unsigned e = 1, k = 0;
  while ((1U << e) < E) {
    ++e;
  }
  while ((1U << k) < K) {
    ++k;
  }
  unsigned n = (8 * E <= 9 * (1U << (e - 1)) && 16 * K < 9 * E) ? e - 1 : e;
  n          = std::min(std::min(n, k + 3), 10U);
  return 1U << std::max(n, 5U);
}

bool block_ok(unsigned A, unsigned E, unsigned* K_out, unsigned* E_out)
{
  const unsigned C = get_nof_uci_codeblocks(A, E), L = get_uci_crc_size(A);
  const unsigned K = (A + C - 1) / C + L, Eb = E / C;
  *K_out = K;
  *E_out = Eb;
  if (K < 18 || (K > 25 && K < 31) || K > 1023 || Eb > 8192) {
    return false;
  }
  return K + (K <= 25 ? 3 : 0) < Eb && K < code_length(K, Eb);
}

bool size_ok(const Size& s)
{
  if (s.A < 1 || s.A > 1706) {
    return false;
  }
  if (s.A <= 2) {
    return s.E >= std::max(s.mod, 1U);
  }
  if (s.A <= 11) {
    return s.E > s.A;
  }
  unsigned K, Eb;
  return block_ok(s.A, s.E, &K, &Eb);
}


} // namespace

int main(int argc, char** argv)
{
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s uci_decoder_configs.json OUTPUT_DIR\n", argv[0]);
    return 1;
  }
  std::vector<Size> sizes;
  {
    std::ifstream     f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    const std::regex  re("\"message_length\": (\\d+), \"llr_length\": (\\d+), \"modulation\": \"(\\w+)\"");
    for (std::sregex_iterator it(text.begin(), text.end(), re), end; it != end; ++it) {
      const std::string m   = (*it)[3];
      const unsigned    mod = m == "PI_2_BPSK" ? 0 : m == "BPSK" ? 1 : m == "QPSK" ? 2 : m == "QAM16" ? 4 : m == "QAM64" ? 6 : 8;
      sizes.push_back({(unsigned)std::stoul((*it)[1]), (unsigned)std::stoul((*it)[2]), mod});
    }
  }
  const size_t nof_configs = sizes.size();
  // The edge sizes.  Parity-check bits (A = 12..19) and their neighbours, E - K below and above 189.
  for (unsigned A = 12; A <= 25; ++A) {
    const unsigned K = A + get_uci_crc_size(A);
    for (unsigned E : {K + 4, K + 20, 100U, K + 189, K + 190, 255U, 256U, 300U, 1000U}) {
      sizes.push_back({A, E, 2});
    }
  }
  // Repetition, puncturing and shortening for every code length: the first two sizes of a grid that fall into each class.
  {
    std::set<unsigned> seen;
    unsigned           count[11][3] = {};
    for (unsigned A : {12U, 16U, 19U, 20U, 25U, 32U, 48U, 64U, 100U, 150U, 200U, 300U, 400U, 500U, 700U, 900U, 1000U}) {
      for (unsigned num : {9U, 10U, 11U, 12U, 14U, 16U, 20U, 24U, 32U, 48U, 64U, 100U}) {
        unsigned E = (A + 11) * num / 8 + 5, K, Eb;
        if (E > 8192 || !block_ok(A, E, &K, &Eb) || get_nof_uci_codeblocks(A, E) != 1) {
          continue;
        }
        const unsigned N = code_length(K, E), mode = E >= N ? 0 : (16 * K <= 7 * E ? 1 : 2);
        unsigned       n = 0;
        while ((1U << n) < N) {
          ++n;
        }
        if (count[n][mode] < 2 && seen.insert(A * 65536 + E).second) {
          ++count[n][mode];
          sizes.push_back({A, E, 2});
        }
      }
    }
  }
  for (Size s : {Size{359, 1088, 2}, Size{360, 1087, 2}, Size{360, 1088, 2}, Size{1012, 2000, 2}, Size{1012, 8192, 2},
                 Size{1013, 1100, 2}, Size{1013, 2000, 2}, Size{1706, 16384, 2}}) {
    sizes.push_back(s);
  }

  uci_decoder_impl decoder(std::make_unique<short_block_detector_impl>(),
                           std::make_unique<polar_code_impl>(),
                           std::make_unique<polar_rate_dematcher_impl>(),
                           std::make_unique<polar_decoder_impl>(std::make_unique<polar_encoder_impl>(), 10),
                           std::make_unique<polar_deallocator_impl>(),
                           std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC6),
                           std::make_unique<crc_calculator_generic_impl>(crc_generator_poly::CRC11));
  short_block_encoder_impl short_encoder;
  polar_code_impl          code;
  polar_allocator_impl     allocator;
  polar_encoder_impl       encoder;
  polar_rate_matcher_impl  rate_matcher;
  crc_calculator_generic_impl  crc6(crc_generator_poly::CRC6), crc11(crc_generator_poly::CRC11);

  std::mt19937                     rng(20240129);
  std::normal_distribution<double> gauss(0.0, 1.0);
  std::vector<int32_t>             cases;
  std::vector<int8_t>              llrs;
  std::vector<uint8_t>             sent, decoded;
  size_t                           skipped = 0;
  for (size_t i = 0; i != sizes.size(); ++i) {
    const Size& s = sizes[i];
    if (!size_ok(s)) {
      if (i < nof_configs) {
        std::fprintf(stderr, "configuration %zu (%u, %u) is refused\n", i, s.A, s.E);
        return 1;
      }
      ++skipped;
      continue;
    }
    // Message and codeword.
    std::vector<uint8_t> msg(s.A), cw(s.E, PLACEHOLDER_ONE);
    for (uint8_t& b : msg) {
      b = (uint8_t)(rng() & 1U);
    }
    if (s.A <= 11) {
      short_encoder.encode(cw, msg, scheme(s.mod));
    } else {
      const unsigned  C = get_nof_uci_codeblocks(s.A, s.E), L = get_uci_crc_size(s.A), Eb = s.E / C;
      crc_calculator& crc = L == 11 ? (crc_calculator&)crc11 : (crc_calculator&)crc6;
      unsigned        first = 0;
      for (unsigned r = 0; r != C; ++r) {
        const unsigned       filler = r == 0 ? s.A % C : 0, len = r == 0 ? s.A / C : (s.A + C - 1) / C;
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
      for (unsigned k = C * Eb; k != s.E; ++k) {
        cw[k] = 0; // bits beyond the blocks are not read by the decoder
      }
    }
    // Thin the largest sizes: noiseless, one noisy and the extreme input only.
    for (int kind = 0; kind != 5; ++kind) {
      if (s.E > 4096 && i < nof_configs && (kind == 2 || kind == 3)) {
        continue;
      }
      std::vector<log_likelihood_ratio> llr(s.E);
      for (unsigned k = 0; k != s.E; ++k) {
        const bool   placeholder = cw[k] > 1;
        const double clean       = placeholder ? 0.0 : (cw[k] ? -20.0 : 20.0);
        int          v           = 0;
        if (kind == 0) {
          v = (int)clean;
        } else if (kind == 1 || kind == 2) {
          v = (int)std::lround(clean + (kind == 1 ? 8.0 : 40.0) * gauss(rng));
          v = std::max(-120, std::min(120, v));
        } else if (kind == 4) {
          v = (rng() & 1U) ? 127 : 120;
          if ((cw[k] == 1) != (rng() % 10 == 0)) {
            v = -v;
          }
        }
        llr[k] = v;
      }
      std::vector<uint8_t> out(s.A, FILL);
      const uci_status     status = decoder.decode(out, llr, {scheme(s.mod)});
      const int32_t        row[8] = {(int32_t)s.A, (int32_t)s.E, (int32_t)s.mod, kind, (int32_t)llrs.size(), (int32_t)sent.size(),
                                     status == uci_status::valid ? 1 : (status == uci_status::invalid ? 2 : 0), 0};
      cases.insert(cases.end(), row, row + 8);
      for (log_likelihood_ratio v : llr) {
        llrs.push_back(v.to_value_type());
      }
      sent.insert(sent.end(), msg.begin(), msg.end());
      decoded.insert(decoded.end(), out.begin(), out.end());
    }
  }
  const std::string dir = argv[2];
  write_npy(dir + "/uci_reference_cases.npy", "<i4", cases, 8);
  write_npy(dir + "/uci_reference_llr.npy", "|i1", llrs, 0);
  write_npy(dir + "/uci_reference_sent.npy", "|u1", sent, 0);
  write_npy(dir + "/uci_reference_decoded.npy", "|u1", decoded, 0);
  std::printf("%zu cases (%zu of the edge sizes refused and left out), %zu soft bits\n", cases.size() / 8, skipped, llrs.size());
  return 0;
}
