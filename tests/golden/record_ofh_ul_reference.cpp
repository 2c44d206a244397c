// Records the answers of srsRAN-5G-ER's Open Fronthaul receive path for tests/test_ofh_uplink.py: the generic decompressors
// (iq_compression_none_impl, iq_compression_bfp_impl -- the SIMD classes delegate decompress to them) on seeded payloads, and
// the two data-flow writers (uplane_rx_symbol_data_flow_writer, uplane_prach_symbol_data_flow_writer) with the test doubles
// of the reference's own unit tests (R/tests/unittests/ofh/receiver/helpers.h, R a checkout of srsRAN-5G-ER) on the section
// ranges those tests use.  Built and run by oracle/recorders.mk, into oracle/_ref/: `make -C oracle recorders`,
// `make -C oracle rerecord-check`; no binary or object is committed.
//
// Inputs are not stored.  With mix the 32-bit finaliser of recorder_io.h, byte k of a payload of seed s is mix(s + k) & 0xFF.
//
// Decompression case i (seed 0x9E3779B9 * (i + 1)): type none with widths 2..16, then BFP with widths 1..16 x udCompParam
// 0..30.  Four PRB records: the packed bytes all 0x00, all 0xFF, the most negative value in every field, seeded (bytes
// k = 0 ... 3 * width - 1 of the case's payload); for BFP every record's udCompParam is the case's.
//   ofh_ul_reference_cases.npy   int64 [n][4]: type, width, udCompParam (-1 for none), first row of the case in prbs
//   ofh_ul_reference_prbs.npy    uint16 [4 n][24]: raw cbf16, re and im of 12 subcarriers
//
// Writer cases (ofh_ul_reference_writers.json): a section's payload is nof_prbs records of the seeded bytes of its seed;
// for BFP the udCompParam byte of each record is its seeded byte & 0x0F.  The section's samples are what the reference's
// decompressor makes of it.  Grid cases are the seven section ranges of ofh_uplane_rx_symbol_data_flow_writer_test.cpp on its
// 51-PRB grid (six tests, the last one writes two sections): the resource elements the context marks as written (first_subc, nof_subc) and their cbf16 words.  PRACH cases are those of
// ofh_uplane_prach_symbol_data_flow_writer_test.cpp for formats 0 and B4 on symbol 0: the context's prach_nof_re and
// offset_to_first_re, the written elements (first_re, nof_re) and the bits of their complex floats.  Every other element of
// the doubles' buffers is checked here to hold what it held before.
//   ofh_ul_reference_writers.npy  uint32: the values of every case, each at its values_offset (one word per grid element, two
//                                 per PRACH element)
#include "helpers.h"
#include "lib/ofh/compression/iq_compression_bfp_impl.h"
#include "lib/ofh/compression/iq_compression_none_impl.h"
#include "lib/ofh/receiver/ofh_uplane_prach_symbol_data_flow_writer.h"
#include "lib/ofh/receiver/ofh_uplane_rx_symbol_data_flow_writer.h"
#include "recorder_io.h"
#include "srsran/ofh/serdes/ofh_message_decoder_properties.h"

using namespace srsran;
using namespace ofh;
using namespace ofh::testing;

namespace {

srslog::basic_logger& logger()
{
  return srslog::fetch_basic_logger("TEST");
}

void decompress(span<cbf16_t> out, span<const compressed_prb> in, unsigned type, unsigned width)
{
  ru_compression_params params;
  params.type       = type == 0 ? compression_type::none : compression_type::BFP;
  params.data_width = width;
  if (type == 0) {
    iq_compression_none_impl(logger(), 1.0F).decompress(out, in, params);
  } else {
    iq_compression_bfp_impl(logger(), 1.0F).decompress(out, in, params);
  }
}

void set_prb(compressed_prb& prb, const uint8_t* packed, unsigned width, unsigned param)
{
  prb.set_compression_param(param);
  std::memcpy(prb.get_byte_buffer().data(), packed, 3 * width);
  prb.set_stored_size(3 * width);
}

struct section_spec {
  unsigned start_prb, nof_prbs, type, width;
  uint32_t seed;
};

// The section's samples: the reference's decompressor on the seeded payload.
void fill_section(uplane_section_params& section, const section_spec& s)
{
  const unsigned              rec = 3 * s.width + s.type;
  std::vector<compressed_prb> prbs(s.nof_prbs);
  std::vector<uint8_t>        bytes(rec);
  for (unsigned p = 0; p != s.nof_prbs; ++p) {
    for (unsigned k = 0; k != rec; ++k) {
      bytes[k] = mix(s.seed + p * rec + k) & 0xFFU;
    }
    set_prb(prbs[p], bytes.data() + s.type, s.width, s.type ? bytes[0] & 0x0FU : 0U);
  }
  section.start_prb = s.start_prb;
  section.nof_prbs  = s.nof_prbs;
  section.iq_samples.resize(s.nof_prbs * NOF_SUBCARRIERS_PER_RB);
  decompress(section.iq_samples, prbs, s.type, s.width);
}

std::string sections_json(const std::vector<section_spec>& sections)
{
  std::ostringstream o;
  o << "[";
  for (size_t i = 0; i != sections.size(); ++i) {
    const section_spec& s = sections[i];
    o << (i ? ", " : "") << "{\"start_prb\": " << s.start_prb << ", \"nof_prbs\": " << s.nof_prbs << ", \"type\": " << s.type
      << ", \"data_width\": " << s.width << ", \"seed\": " << s.seed << "}";
  }
  o << "]";
  return o.str();
}

uint32_t bits(float v)
{
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

int fail(const char* what, const char* name)
{
  std::fprintf(stderr, "%s: %s\n", name, what);
  return 1;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 1;
  }
  const std::string out = argv[1];

  // ---- decompression ----
  std::vector<int64_t>  cases;
  std::vector<uint16_t> prbs_out;
  unsigned              index = 0;
  for (unsigned type = 0; type != 2; ++type) {
    for (unsigned width = type ? 1 : 2; width != 17; ++width) {
      for (unsigned param = 0; param != (type ? 31U : 1U); ++param) {
        const uint32_t seed = 0x9E3779B9U * (index + 1);
        uint8_t        packed[4][48];
        std::memset(packed[0], 0x00, 48);
        std::memset(packed[1], 0xFF, 48);
        std::memset(packed[2], 0x00, 48);
        for (unsigned v = 0; v != 24; ++v) { // the sign bit of every field
          const unsigned bit = v * width;
          packed[2][bit / 8] |= 0x80U >> (bit % 8);
        }
        for (unsigned k = 0; k != 3 * width; ++k) {
          packed[3][k] = mix(seed + k) & 0xFFU;
        }
        std::vector<compressed_prb> in(4);
        for (unsigned p = 0; p != 4; ++p) {
          set_prb(in[p], packed[p], width, param);
        }
        std::vector<cbf16_t> res(4 * NOF_SUBCARRIERS_PER_RB);
        decompress(res, in, type, width);
        cases.insert(cases.end(), {(int64_t)type, (int64_t)width, type ? (int64_t)param : -1, (int64_t)(prbs_out.size() / 24)});
        const uint16_t* raw = reinterpret_cast<const uint16_t*>(res.data());
        prbs_out.insert(prbs_out.end(), raw, raw + 4 * 24);
        ++index;
      }
    }
  }
  write_npy(out + "/ofh_ul_reference_cases.npy", "<i8", cases, 4);
  write_npy(out + "/ofh_ul_reference_prbs.npy", "<u2", prbs_out, 24);

  // ---- the resource-grid writer ----
  std::vector<uint32_t> values;
  std::ostringstream    json;
  json << "{\n \"grid_nof_prbs\": 51,\n \"grid\": [\n";
  struct grid_case {
    const char*               name;
    std::vector<section_spec> sections; // written one after the other
  };
  const std::vector<grid_case> grid_cases = {
      {"decoded_prbs_outside_grid_prbs_do_not_write", {{51, 50, 1, 9, 101}}},
      {"decoded_prbs_match_grid_prbs_write", {{0, 51, 0, 16, 102}}},
      {"decoded_prbs_bigger_than_grid_prbs_write", {{0, 273, 1, 14, 103}}},
      {"segmented_prbs_inside_the_grid_write", {{0, 10, 0, 2, 104}}},
      {"segmented_prbs_write_the_prbs_overlapped_with_grid", {{40, 60, 1, 12, 105}}},
      {"segmented_prbs_fill_the_grid", {{0, 50, 0, 8, 106}, {50, 1, 1, 16, 107}}},
  };
  const static_vector<unsigned, MAX_NOF_SUPPORTED_EAXC> ul_eaxc = {0, 1, 2, 3};
  for (size_t c = 0; c != grid_cases.size(); ++c) {
    const grid_case&                           gc   = grid_cases[c];
    std::shared_ptr<uplink_context_repository> repo = std::make_shared<uplink_context_repository>(1);
    const slot_point                           slot(0, 0, 1);
    resource_grid_writer_bool_spy              rg_writer(MAX_NOF_PRBS);
    resource_grid_dummy_with_spy_writer        grid(rg_writer);
    uplane_rx_symbol_data_flow_writer          writer(ul_eaxc, logger(), repo);
    uplane_message_decoder_results             results;
    results.params.slot      = slot;
    results.params.symbol_id = 0;
    results.sections.emplace_back();
    repo->add({slot, 0}, grid, {0, 14});
    for (const section_spec& s : gc.sections) {
      fill_section(results.sections.back(), s);
      writer.write_to_resource_grid(ul_eaxc[0], results);
    }
    uplink_context context = repo->get(slot, 0);
    const auto&    mask    = context.get_re_written_mask()[0];
    span<cbf16_t>  view    = rg_writer.get_view(0, 0);
    const cbf16_t  untouched{-1.0, +1.0};
    unsigned       first = 0, count = 0;
    for (unsigned k = 0; k != view.size(); ++k) {
      const bool written = k < mask.size() && mask.test(k);
      if (written && count == 0) {
        first = k;
      }
      if (written && count != 0 && k != first + count) {
        return fail("the written elements are not one range", gc.name);
      }
      count += written;
      if (!written && view[k] != untouched) {
        return fail("an element outside the written range changed", gc.name);
      }
    }
    json << "  {\"name\": \"" << gc.name << "\", \"sections\": " << sections_json(gc.sections) << ", \"first_subc\": " << first
         << ", \"nof_subc\": " << count << ", \"values_offset\": " << values.size() << "}" << (c + 1 != grid_cases.size() ? "," : "") << "\n";
    for (unsigned k = first; k != first + count; ++k) {
      uint32_t w;
      std::memcpy(&w, &view[k], 4);
      values.push_back(w);
    }
  }
  json << " ],\n \"prach\": [\n";

  // ---- the PRACH writer ----
  struct prach_case {
    const char*        name;
    prach_format_type  format;
    subcarrier_spacing pusch_scs;
    section_spec       section;
  };
  const prach_format_type  F0 = prach_format_type::zero, B4 = prach_format_type::B4;
  const subcarrier_spacing k30 = subcarrier_spacing::kHz30, k60 = subcarrier_spacing::kHz60;
  const std::vector<prach_case> prach_cases = {
      {"decoded_prbs_outside_prach_prbs_do_not_write/0", F0, k30, {100, 50, 1, 9, 201}},
      {"decoded_prbs_outside_prach_prbs_do_not_write/B4", B4, k30, {100, 50, 0, 16, 202}},
      {"decoded_prbs_before_prach_prbs_do_not_write", F0, k60, {0, 11, 1, 9, 203}},
      {"prbs_at_the_beginning_write_the_expected_re", F0, k60, {11, 1, 1, 14, 204}},
      {"60kHz_long_format_one_message", F0, k60, {0, 81, 1, 9, 205}},
      {"60kHz_long_format_one_message_all_prbs", F0, k60, {0, 96, 0, 12, 206}},
      {"decoded_prbs_in_one_packet_passes/0", F0, k30, {0, 72, 1, 9, 207}},
      {"decoded_prbs_in_one_packet_passes/B4", B4, k30, {0, 12, 1, 9, 208}},
      {"prach_in_three_message_first_message/0", F0, k30, {0, 24, 1, 9, 209}},
      {"prach_in_three_message_second_message/0", F0, k30, {24, 24, 0, 16, 210}},
      {"prach_in_three_message_third_message/0", F0, k30, {48, 24, 1, 12, 211}},
      {"prach_in_three_message_first_message/B4", B4, k30, {0, 4, 1, 9, 212}},
      {"prach_in_three_message_second_message/B4", B4, k30, {4, 4, 0, 9, 213}},
      {"prach_in_three_message_third_message/B4", B4, k30, {8, 4, 1, 16, 214}},
  };
  const static_vector<unsigned, MAX_NOF_SUPPORTED_EAXC> prach_eaxc = {4, 5, 6, 7};
  for (size_t c = 0; c != prach_cases.size(); ++c) {
    const prach_case&                         pc   = prach_cases[c];
    std::shared_ptr<prach_context_repository> repo = std::make_shared<prach_context_repository>(1);
    const slot_point                          slot(0, 0, 1);
    prach_buffer_dummy                        buffer(get_preamble_duration(pc.format), is_long_preamble(pc.format));
    prach_buffer_context                      buffer_context;
    buffer_context.slot             = slot;
    buffer_context.format           = pc.format;
    buffer_context.ports            = {0};
    buffer_context.nof_td_occasions = 1;
    buffer_context.nof_fd_occasions = 1;
    buffer_context.pusch_scs        = pc.pusch_scs;
    buffer_context.start_symbol     = 0;
    repo->add(buffer_context, buffer, std::nullopt, std::nullopt);
    span<cf_t>  symbols = buffer.get_symbol(0, 0, 0, 0);
    const cf_t untouched(-7.0F, 7.0F);
    std::fill(symbols.begin(), symbols.end(), untouched);
    uplane_prach_symbol_data_flow_writer writer(prach_eaxc, logger(), repo);
    uplane_message_decoder_results       results;
    results.params.slot      = slot;
    results.params.symbol_id = 0;
    results.sections.emplace_back();
    fill_section(results.sections.back(), pc.section);
    writer.write_to_prach_buffer(prach_eaxc[0], results);
    prach_context context = repo->get(slot);
    const auto&   mask    = context.get_symbol_re_written(0)[0];
    unsigned      first = 0, count = 0;
    for (unsigned k = 0; k != symbols.size(); ++k) {
      const bool written = k < mask.size() && mask.test(k);
      if (written && count == 0) {
        first = k;
      }
      if (written && count != 0 && k != first + count) {
        return fail("the written elements are not one range", pc.name);
      }
      count += written;
      if (!written && symbols[k] != untouched) {
        return fail("an element outside the written range changed", pc.name);
      }
    }
    json << "  {\"name\": \"" << pc.name << "\", \"format\": \"" << (pc.format == F0 ? "0" : "B4")
         << "\", \"pusch_scs_khz\": " << (pc.pusch_scs == k30 ? 30 : 60) << ", \"sections\": " << sections_json({pc.section})
         << ", \"prach_nof_re\": " << context.get_prach_nof_re() << ", \"offset_to_first_re\": " << context.get_prach_offset_to_first_re()
         << ", \"first_re\": " << first << ", \"nof_re\": " << count << ", \"values_offset\": " << values.size() << "}"
         << (c + 1 != prach_cases.size() ? "," : "") << "\n";
    for (unsigned k = first; k != first + count; ++k) {
      values.push_back(bits(symbols[k].real()));
      values.push_back(bits(symbols[k].imag()));
    }
  }
  json << " ]\n}\n";
  std::ofstream(out + "/ofh_ul_reference_writers.json") << json.str();
  write_npy(out + "/ofh_ul_reference_writers.npy", "<u4", values, 0);
  std::printf("%u decompression cases, %zu grid cases, %zu PRACH cases, %zu words\n", index, grid_cases.size(), prach_cases.size(),
              values.size());
  return 0;
}
