// Records the Ethernet frames of srsRAN-5G-ER's Open Fronthaul downlink user-plane data flow for tests/test_ofh_downlink.py:
// the real data_flow_uplane_downlink_data_impl with the real VLAN Ethernet and eCPRI builders, the static and the dynamic
// user-plane message builders, the AVX2 compressors (the ones nrphy_ofh_compress is pinned to) and an eth_frame_pool of the
// case's MTU, reading a seeded grid through a plain resource_grid_reader.  Built and run by oracle/recorders.mk, against a
// checkout of srsRAN-5G-ER and into oracle/_ref/: `make -C oracle recorders`, `make -C oracle rerecord-check`; no binary or
// object is committed.  The recipe builds this file with -fno-access-control, for one line: the data flow's sequence generator
// always starts at 0, and the case with sequence identifiers 254, 255, 0 sets its counter.
//
// Grids are not stored.  With mix the 32-bit finaliser of recorder_io.h, value i (i = ((port * 14 + symbol) * nof_subc + k) * 2 + re/im)
// of the grid of seed s comes from h = mix(s + i) and the class c = mix(31 s + k / 12 + 0x51ED) & 3 of its PRB:
//   magnitude  (h >> 4) & 31                    if (h & 15) < 12 or c < 2     small integers
//              64 * ((h >> 4) & 127)            else if (h & 15) < 14 or c == 2
//              8192 * (1 + ((h >> 4) & 7))      else
//   negative if h >> 31.  Every magnitude is exact in bf16.  Each case's iq_scaling is the float s nearest to 2.5 / gain with
// float(gain * s) == 2.5 exactly (gain = 2^(width - 1) - 1, 32767 for BFP), so the quantiser multiplies by 2.5: odd values
// land on x.5, where the vector loop's round-to-even and the tail's round-half-away differ, and magnitudes from 16384 on leave
// the int16 range, where the vector loop saturates and the tail wraps.
//
//   ofh_dl_reference_cases.json   per case the flow, the grid, the descriptors and, per descriptor, its frames: start_prb,
//                                 nof_prbs, frame_bytes (frame_buffer::size()), offset of the frame's bytes in the .npy
//   ofh_dl_reference_frames.npy   uint8: the bytes of every frame, back to back
#include "lib/ofh/compression/iq_compression_bfp_avx2.h"
#include "lib/ofh/compression/iq_compression_none_avx2.h"
#include "lib/ofh/ecpri/ecpri_packet_builder_impl.h"
#include "lib/ofh/ethernet/vlan_ethernet_frame_builder_impl.h"
#include "lib/ofh/serdes/ofh_uplane_message_builder_dynamic_compression_impl.h"
#include "lib/ofh/serdes/ofh_uplane_message_builder_static_compression_impl.h"
#include "lib/ofh/transmitter/ofh_data_flow_uplane_downlink_data_impl.h"
#include "recorder_io.h"
#include "srsran/ofh/ethernet/ethernet_frame_pool.h"
#include "srsran/phy/support/resource_grid_reader.h"

#include <cmath>

using namespace srsran;
using namespace ofh;

namespace {

// A seeded grid [ports][14][nof_subc] behind the reference's reader interface.
class seeded_grid : public resource_grid_reader
{
  unsigned             ports, nof_subc;
  std::vector<cbf16_t> data;

public:
  seeded_grid(uint32_t seed, unsigned ports_, unsigned nof_subc_) : ports(ports_), nof_subc(nof_subc_), data(ports_ * 14 * nof_subc_)
  {
    for (unsigned re = 0; re != data.size(); ++re) {
      const uint32_t cls = mix(31U * seed + (re % nof_subc) / 12U + 0x51EDU) & 3U;
      float          v[2];
      for (unsigned c = 0; c != 2; ++c) {
        const uint32_t h = mix(seed + 2U * re + c), sel = h & 15U, m = h >> 4;
        float          mag;
        if (sel < 12 || cls < 2) {
          mag = float(m & 31U);
        } else if (sel < 14 || cls == 2) {
          mag = 64.0F * float(m & 127U);
        } else {
          mag = 8192.0F * float(1U + (m & 7U));
        }
        v[c] = (h >> 31) ? -mag : mag;
      }
      data[re] = cbf16_t(v[0], v[1]);
    }
  }
  unsigned   get_nof_ports() const override { return ports; }
  unsigned   get_nof_subc() const override { return nof_subc; }
  unsigned   get_nof_symbols() const override { return 14; }
  bool       is_empty(unsigned) const override { return false; }
  bool       is_empty() const override { return false; }
  span<cf_t> get(span<cf_t> symbols, unsigned, unsigned, unsigned, const bounded_bitset<MAX_RB * NRE>&) const override { return symbols; }
  span<cbf16_t> get(span<cbf16_t> symbols, unsigned, unsigned, unsigned, const bounded_bitset<MAX_RB * NRE>&) const override
  {
    return symbols;
  }
  void get(span<cf_t>, unsigned, unsigned, unsigned, unsigned) const override {}
  void get(span<cbf16_t> symbols, unsigned port, unsigned l, unsigned k_init) const override
  {
    std::memcpy(symbols.data(), &data[(port * 14 + l) * nof_subc + k_init], symbols.size() * sizeof(cbf16_t));
  }
  span<const cbf16_t> get_view(unsigned port, unsigned l) const override { return {&data[(port * 14 + l) * nof_subc], nof_subc}; }
};

float scaling_for(unsigned type, unsigned width)
{
  const float gain = float((1 << ((type ? 16 : width) - 1)) - 1);
  float       s    = 2.5F / gain;
  for (int step = 0; step != 64; ++step) {
    float up = s, down = s;
    for (int k = 0; k != step; ++k) {
      up   = std::nextafterf(up, 1.0F);
      down = std::nextafterf(down, 0.0F);
    }
    volatile float a = gain * up, b = gain * down;
    if (a == 2.5F) {
      return up;
    }
    if (b == 2.5F) {
      return down;
    }
  }
  std::fprintf(stderr, "no scaling for type %u width %u\n", type, width);
  std::exit(1);
}

struct symbol_spec {
  unsigned port, eaxc, symbol, seq_id;
};

struct case_spec {
  const char*              name;
  unsigned                 mtu, ru_nof_prbs, static_compression, type, width, grid_nof_subc, grid_ports;
  uint32_t                 seed;
  unsigned                 numerology, sfn, subframe, slot;
  std::vector<symbol_spec> symbols; // consecutive symbols are recorded in one call when they start at 0
};

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 1;
  }
  const std::string           out = argv[1];
  srslog::basic_logger&       logger = srslog::fetch_basic_logger("TEST");
  const std::vector<case_spec> cases = {
      {"a_unit_test_none16_two_fragments", 9000, 273, 1, 0, 16, 3276, 1, 11, 1, 0, 0, 0, {{0, 2, 13, 0}}},
      {"b_bfp9_one_fragment_of_273", 9000, 273, 1, 1, 9, 3276, 1, 12, 1, 1023, 9, 1, {{0, 0, 0, 200}}},
      {"c_bfp12_dynamic_mtu1500_106", 1500, 106, 0, 1, 12, 1272, 2, 13, 1, 5, 3, 0, {{1, 1, 6, 17}}},
      {"c_bfp12_static_mtu1500_106", 1500, 106, 1, 1, 12, 1272, 2, 13, 1, 5, 3, 0, {{1, 1, 6, 17}}},
      {"d_none16_mtu1500_273", 1500, 273, 1, 0, 16, 3276, 1, 14, 0, 300, 4, 0, {{0, 3, 7, 99}}},
      {"e_none8_static_one_prb", 1500, 1, 1, 0, 8, 12, 1, 15, 1, 1, 1, 1, {{0, 0, 2, 1}}},
      {"e_none8_dynamic_one_prb", 1500, 1, 0, 0, 8, 12, 1, 15, 1, 1, 1, 1, {{0, 0, 2, 1}}},
      {"f_mtu_of_headers_and_one_record", 82, 4, 1, 0, 16, 48, 1, 16, 1, 2, 2, 0, {{0, 1, 4, 7}}},
      {"g_ru_25_prbs_over_a_240_subcarrier_grid", 1500, 25, 1, 1, 9, 240, 2, 17, 1, 64, 0, 1, {{1, 0, 9, 0}}},
      {"h_sequence_wraps", 1500, 106, 1, 1, 12, 1272, 1, 18, 1, 511, 8, 0, {{0, 31, 3, 254}}},
      {"j_three_symbols_sfn_777", 800, 51, 0, 1, 9, 612, 2, 19, 3, 777, 7, 5, {{1, 3, 0, 40}, {1, 3, 1, 42}, {1, 3, 2, 44}}},
      {"k_none12_dynamic_two_fragments", 600, 30, 0, 0, 12, 360, 1, 20, 1, 0, 0, 0, {{0, 0, 11, 255}}},
  };

  std::vector<uint8_t> bytes;
  std::ostringstream   json;
  json << "[\n";
  for (size_t c = 0; c != cases.size(); ++c) {
    const case_spec& cs = cases[c];
    const float      iq_scaling = scaling_for(cs.type, cs.width);
    uint32_t         scaling_bits;
    std::memcpy(&scaling_bits, &iq_scaling, 4);

    data_flow_uplane_downlink_data_impl_config config;
    config.cp                      = cyclic_prefix::NORMAL;
    config.ru_nof_prbs             = cs.ru_nof_prbs;
    config.vlan_params             = {{0xaa, 0xbb, 0xcc, 0xdd, 0xee, uint8_t(0x11 + c)}, {0x02, 0x42, 0x0a, 0x00, uint8_t(c), 0x22}, uint16_t(0x2000 + 7 * c), 0xaefe};
    config.compr_params.type       = cs.type ? compression_type::BFP : compression_type::none;
    config.compr_params.data_width = cs.width;
    config.dl_eaxc.push_back(cs.symbols.front().eaxc);

    std::unique_ptr<iq_compressor> compressor;
    if (cs.type) {
      compressor = std::make_unique<iq_compression_bfp_avx2>(logger, iq_scaling);
    } else {
      compressor = std::make_unique<iq_compression_none_avx2>(logger, iq_scaling);
    }
    const unsigned                         frames_per_symbol = 16;
    std::shared_ptr<ether::eth_frame_pool> pool = std::make_shared<ether::eth_frame_pool>(units::bytes(cs.mtu), frames_per_symbol);

    data_flow_uplane_downlink_data_impl_dependencies deps;
    deps.logger        = &logger;
    deps.frame_pool    = pool;
    deps.eth_builder   = std::make_unique<ether::vlan_frame_builder_impl>();
    deps.ecpri_builder = std::make_unique<ecpri::packet_builder_impl>();
    if (cs.static_compression) {
      deps.up_builder = std::make_unique<ofh_uplane_message_builder_static_compression_impl>(logger, *compressor);
    } else {
      deps.up_builder = std::make_unique<ofh_uplane_message_builder_dynamic_compression_impl>(logger, *compressor);
    }
    deps.compressor_sel = std::move(compressor);
    data_flow_uplane_downlink_data_impl flow(config, std::move(deps));

    seeded_grid      grid(cs.seed, cs.grid_ports, cs.grid_nof_subc);
    const slot_point slot(cs.numerology, cs.sfn, cs.subframe, cs.slot);

    json << " {\"name\": \"" << cs.name << "\", \"mtu\": " << cs.mtu << ", \"ru_nof_prbs\": " << cs.ru_nof_prbs
         << ", \"static_compression\": " << cs.static_compression << ", \"type\": " << cs.type << ", \"data_width\": " << cs.width
         << ", \"iq_scaling_bits\": " << scaling_bits << ", \"mac_dst\": [";
    for (unsigned k = 0; k != 6; ++k) {
      json << (k ? ", " : "") << unsigned(config.vlan_params.mac_dst_address[k]);
    }
    json << "], \"mac_src\": [";
    for (unsigned k = 0; k != 6; ++k) {
      json << (k ? ", " : "") << unsigned(config.vlan_params.mac_src_address[k]);
    }
    json << "], \"tci\": " << config.vlan_params.tci << ", \"eth_type\": " << config.vlan_params.eth_type
         << ", \"grid_nof_subc\": " << cs.grid_nof_subc << ", \"grid_ports\": " << cs.grid_ports << ", \"seed\": " << cs.seed
         << ", \"sfn\": " << cs.sfn << ", \"subframe\": " << cs.subframe << ", \"slot\": " << cs.slot << ",\n  \"symbols\": [\n";

    // One call per run of symbols.  The reference's loop ends at symbol_range.length(), so a call for symbols
    // [first, first + n) passes a range of that start and of length first + n.
    const unsigned first = cs.symbols.front().symbol, count = cs.symbols.size();
    flow.up_seq_gen.counters[cs.symbols.front().eaxc] = uint8_t(cs.symbols.front().seq_id);
    data_flow_uplane_resource_grid_context context;
    context.slot         = slot;
    context.sector       = 0;
    context.port         = cs.symbols.front().port;
    context.eaxc         = cs.symbols.front().eaxc;
    context.symbol_range = {first, 2 * first + count};
    if (context.symbol_range.length() != first + count) {
      std::fprintf(stderr, "%s: symbol range\n", cs.name);
      return 1;
    }
    flow.enqueue_section_type_1_message(context, grid);

    for (size_t i = 0; i != cs.symbols.size(); ++i) {
      const symbol_spec&        s = cs.symbols[i];
      ether::frame_pool_context pc{{message_type::user_plane, data_direction::downlink}, slot_symbol_point(slot, s.symbol, 14)};
      span<const ether::frame_buffer*> frames = pool->read_frame_buffers(pc);
      if (frames.empty() || s.symbol != first + i || s.port != context.port || s.eaxc != context.eaxc) {
        std::fprintf(stderr, "%s: no frames for symbol %u\n", cs.name, s.symbol);
        return 1;
      }
      json << "   {\"port\": " << s.port << ", \"eaxc\": " << s.eaxc << ", \"symbol\": " << s.symbol << ", \"seq_id\": " << s.seq_id
           << ", \"frames\": [";
      unsigned start_prb = 0;
      for (size_t f = 0; f != frames.size(); ++f) {
        span<const uint8_t> d = frames[f]->data();
        // the section header's startPrbu and numPrbu (0: more than 255, then from the length)
        const unsigned hdr = 18 + 8 + (cs.static_compression ? 8 : 10), rec = 3 * cs.width + cs.type, used = d.size();
        const unsigned nof_prbs = d[33] != 0 ? d[33] : (used - hdr) / rec;
        if (start_prb != (((d[31] & 3U) << 8) | d[32]) || used != std::max(64U, hdr + nof_prbs * rec)) {
          std::fprintf(stderr, "%s: frame %zu of symbol %u is not what its header says\n", cs.name, f, s.symbol);
          return 1;
        }
        json << (f ? ", " : "") << "{\"start_prb\": " << start_prb << ", \"nof_prbs\": " << nof_prbs << ", \"frame_bytes\": " << used
             << ", \"offset\": " << bytes.size() << "}";
        start_prb += nof_prbs;
        bytes.insert(bytes.end(), d.begin(), d.end());
      }
      if (start_prb != cs.ru_nof_prbs) {
        std::fprintf(stderr, "%s: the frames of symbol %u hold %u PRBs\n", cs.name, s.symbol, start_prb);
        return 1;
      }
      json << "]}" << (i + 1 != cs.symbols.size() ? "," : "") << "\n";
    }
    json << "  ]}" << (c + 1 != cases.size() ? "," : "") << "\n";
  }
  json << "]\n";
  std::ofstream(out + "/ofh_dl_reference_cases.json") << json.str();
  write_npy(out + "/ofh_dl_reference_frames.npy", bytes);
  std::printf("%zu cases, %zu bytes of frames\n", cases.size(), bytes.size());
  return 0;
}
