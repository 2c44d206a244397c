// Records what srsRAN-5G-ER's Open Fronthaul receiver does with Ethernet frames, for tests/test_ofh_frame_receiver.py.  Every
// frame goes through message_receiver_impl::on_new_frame itself, constructed with the reference's own vlan_frame_decoder_impl,
// packet_decoder_use_header_payload_size or packet_decoder_ignore_header_payload_size, sequence_id_checker_impl, the static
// or the dynamic uplane_message_decoder over an iq_decompressor_selector of the generic decompressors, and
// data_flow_uplane_uplink_data_impl with real uplink_cplane_context_repository and uplink_context_repository.  Thin
// forwarding wrappers around the injected parts note how far a frame got; the grid double (over the doubles of
// R/tests/unittests/ofh/receiver/helpers.h) keeps [ports][14][subcarriers] and is poisoned before every frame, so every write
// shows.  The PRACH data flow is a spy, as in the reference's ofh_message_receiver_test.cpp: the library reports PRACH messages
// and leaves them to the caller.  Built and run by oracle/recorders.mk, against a checkout R of srsRAN-5G-ER and into
// oracle/_ref/: `make -C oracle recorders`, `make -C oracle rerecord-check`; no binary or object is committed.
//
// Four batches: eCPRI payload size used or ignored x static (BFP 9 / none 16) or dynamic compression.  The RU has 9 PRBs, the
// grids 2 ports x 14 x 72 subcarriers (6 PRBs); ul_eaxc = {4, 5}, prach_eaxc = {0, 1}; 30 kHz.  A batch is one receiver and one
// list of frames taken in order.  The frames are built here: PRB records are seeded bytes (mix of recorder_io.h; for BFP the udCompParam
// byte & 0x0F), everything else is stated per frame.  Inputs for which the library defines rules of its own are not fed: an
// eCPRI payload size below 4, dynamic compression types 2..6, none with 1 bit.  No symbol is ever written completely on both
// ports (checked: the notifier is never called), so the contexts the batch starts with stay.
//   ofh_rx_reference_frames.npy   uint8: all frames back to back
//   ofh_rx_reference_cases.json   per batch: the configuration, the expectations (what the two repositories hold) and per frame
//                                 its name, byte range and what the reference did: eth (0 dropped as too short, 1 dropped by the
//                                 address/type filter, 2 passed), ecpri (-1 not reached, 0 the decoder returned nothing, 1
//                                 filtered by message type or eAxC, 2 passed), seq (null: the checker was not asked, else its
//                                 answer), flow (0 none, 1 uplink data, 2 PRACH), decoded (-1 the decoder was not asked, 0 it
//                                 refused, 1 it decoded), write (null or grid, port, symbol, first_subc, nof_subc, values_offset)
//   ofh_rx_reference_values.npy   uint32: the cbf16 words of every write
#include "helpers.h"
#include "lib/ofh/compression/iq_compression_bfp_impl.h"
#include "lib/ofh/compression/iq_compression_death_impl.h"
#include "lib/ofh/compression/iq_compression_none_impl.h"
#include "lib/ofh/compression/iq_decompressor_selector.h"
#include "lib/ofh/ecpri/ecpri_packet_decoder_impl.h"
#include "lib/ofh/ethernet/vlan_ethernet_frame_decoder_impl.h"
#include "lib/ofh/receiver/ofh_data_flow_uplane_uplink_data_impl.h"
#include "lib/ofh/receiver/ofh_message_receiver.h"
#include "lib/ofh/receiver/ofh_rx_window_checker.h"
#include "lib/ofh/receiver/ofh_sequence_id_checker_impl.h"
#include "lib/ofh/serdes/ofh_uplane_message_decoder_dynamic_compression_impl.h"
#include "lib/ofh/serdes/ofh_uplane_message_decoder_static_compression_impl.h"
#include "recorder_io.h"
#include "srsran/ofh/ethernet/ethernet_unique_buffer.h"
#include "tests/unittests/ofh/ofh_uplane_rx_symbol_notifier_test_doubles.h"

using namespace srsran;
using namespace ofh;
using namespace ofh::testing;

namespace {

srslog::basic_logger& logger()
{
  return srslog::fetch_basic_logger("TEST");
}

constexpr unsigned GRID_PORTS = 2, GRID_SUBC = 72, RU_PRBS = 9;
const uint8_t      MAC_DST[6] = {0x00, 0x11, 0x22, 0x33, 0x44, 0x55}, MAC_SRC[6] = {0x66, 0x77, 0x88, 0x99, 0xAA, 0xBB};
constexpr uint16_t ETH_TYPE   = 0xAEFE;
const cbf16_t      POISON{-3.0, +5.0}; // no sample is: |value| <= 32768 / 32767

// ---- what the receiver is built from, each part noting what it was asked and what it answered ----
struct trace {
  int  eth = 0, ecpri = -1, flow = 0, decoded = -1, seq = 0;
  bool seq_asked = false, notified = false;
};
trace now;

class vlan_decoder_wrap : public ether::vlan_frame_decoder
{
  ether::vlan_frame_decoder_impl impl{logger()};

public:
  span<const uint8_t> decode(span<const uint8_t> frame, ether::vlan_frame_params& params) override
  {
    span<const uint8_t> out = impl.decode(frame, params);
    now.eth                 = out.empty() ? 0 : 1; // 2 once the eCPRI decoder is asked
    return out;
  }
};

class ecpri_decoder_wrap : public ecpri::packet_decoder
{
  std::unique_ptr<ecpri::packet_decoder> impl;

public:
  explicit ecpri_decoder_wrap(bool ignore_size)
  {
    if (ignore_size) {
      impl = std::make_unique<ecpri::packet_decoder_ignore_header_payload_size>(logger());
    } else {
      impl = std::make_unique<ecpri::packet_decoder_use_header_payload_size>(logger());
    }
  }
  span<const uint8_t> decode(span<const uint8_t> packet, ecpri::packet_parameters& params) override
  {
    now.eth                 = 2;
    span<const uint8_t> out = impl->decode(packet, params);
    now.ecpri               = out.empty() ? 0 : 1; // 2 once the checker is asked
    return out;
  }
};

class checker_wrap : public sequence_id_checker
{
  sequence_id_checker_impl impl;

public:
  int update_and_compare_seq_id(unsigned eaxc, uint8_t seq_id) override
  {
    now.ecpri     = 2;
    now.seq_asked = true;
    now.seq       = impl.update_and_compare_seq_id(eaxc, seq_id);
    return now.seq;
  }
};

class uplane_decoder_wrap : public uplane_message_decoder
{
  std::unique_ptr<uplane_message_decoder> impl;

public:
  explicit uplane_decoder_wrap(std::unique_ptr<uplane_message_decoder> impl_) : impl(std::move(impl_)) {}
  bool decode(uplane_message_decoder_results& results, span<const uint8_t> message) override
  {
    const bool ok = impl->decode(results, message);
    now.decoded   = ok ? 1 : 0;
    return ok;
  }
};

class data_flow_wrap : public data_flow_uplane_uplink_data
{
  std::unique_ptr<data_flow_uplane_uplink_data> impl;

public:
  explicit data_flow_wrap(std::unique_ptr<data_flow_uplane_uplink_data> impl_) : impl(std::move(impl_)) {}
  void decode_type1_message(unsigned eaxc, span<const uint8_t> message) override
  {
    now.flow = 1;
    impl->decode_type1_message(eaxc, message);
  }
};

class prach_flow_spy : public data_flow_uplane_uplink_prach
{
public:
  void decode_type1_message(unsigned eaxc, span<const uint8_t> message) override { now.flow = 2; }
};

class notifier_spy : public uplane_rx_symbol_notifier
{
public:
  void on_new_uplink_symbol(const uplane_rx_symbol_context& context, const resource_grid_reader& grid) override { now.notified = true; }
  void on_new_prach_window_data(const prach_buffer_context& context, const prach_buffer& buffer) override { now.notified = true; }
};

class eth_receiver_dummy : public ether::receiver
{
  void start(ether::frame_notifier& notifier) override {}
  void stop() override {}
};

class rx_buffer_of : public ether::rx_buffer
{
  std::vector<uint8_t> bytes;

public:
  explicit rx_buffer_of(std::vector<uint8_t> bytes_) : bytes(std::move(bytes_)) {}
  span<const uint8_t> data() const override { return bytes; }
};

// The grid double: the helpers' writer with a store of [ports][14][subcarriers] behind get_view.
class grid_writer : public resource_grid_writer_bool_spy
{
public:
  std::vector<cbf16_t> store = std::vector<cbf16_t>(GRID_PORTS * 14 * GRID_SUBC, POISON);
  unsigned             get_nof_ports() const override { return GRID_PORTS; }
  unsigned             get_nof_subc() const override { return GRID_SUBC; }
  span<cbf16_t>        get_view(unsigned port, unsigned l) override
  {
    return span<cbf16_t>(store).subspan((port * 14 + l) * GRID_SUBC, GRID_SUBC);
  }
};

std::unique_ptr<iq_decompressor> make_decompressor()
{
  std::array<std::unique_ptr<iq_decompressor>, NOF_COMPRESSION_TYPES_SUPPORTED> d;
  d[0] = std::make_unique<iq_compression_none_impl>(logger(), 1.0F);
  d[1] = std::make_unique<iq_compression_bfp_impl>(logger(), 1.0F);
  for (unsigned k = 2; k != NOF_COMPRESSION_TYPES_SUPPORTED; ++k) {
    d[k] = std::make_unique<iq_compression_death_impl>(); // as the reference's factory does: never reached here
  }
  return std::make_unique<iq_decompressor_selector>(std::move(d));
}

// ---- frames ----
struct section_spec {
  unsigned start_prb = 2, nof_prbs_field = 3, records = 3; // records present in the frame
  unsigned type = 1, width = 9;                            // of the records; the udCompHdr under dynamic compression
  unsigned rb = 0, sym_inc = 0, cut = 0;                   // cut: bytes missing at the end of the records
  uint32_t seed = 1;
};

struct frame_spec {
  std::string name;
  bool        bad_dst = false, bad_src = false;
  unsigned    eth_type = ETH_TYPE, revision = 1, concatenation = 0, msg_type = 0;
  int         size_delta = 0; // added to the eCPRI payload size
  unsigned    eaxc = 4, seq = 0;
  unsigned    direction = 0, version = 1, filter = 0, sfn8 = 7, subframe = 3, slot = 1, symbol = 3;
  unsigned    message_bytes = ~0U; // the message cut to this many bytes (sections dropped)
  unsigned    length        = 0;   // the whole frame cut to this many bytes
  std::vector<section_spec> sections = {section_spec{}};
};

struct config {
  const char* name;
  bool        ignore_size, static_compression;
  unsigned    type, width; // static compression: of both routes
};

std::vector<uint8_t> build(const frame_spec& f, const config& c)
{
  std::vector<uint8_t> m = {(uint8_t)(f.direction << 7 | f.version << 4 | f.filter), (uint8_t)f.sfn8,
                            (uint8_t)(f.subframe << 4 | f.slot >> 2), (uint8_t)((f.slot & 3U) << 6 | f.symbol)};
  for (const section_spec& s : f.sections) {
    m.insert(m.end(), {0x00, (uint8_t)(0x10 | s.rb << 3 | s.sym_inc << 2 | (s.start_prb >> 8 & 3U)), (uint8_t)s.start_prb, (uint8_t)s.nof_prbs_field});
    if (!c.static_compression) {
      m.insert(m.end(), {(uint8_t)((s.width & 0xFU) << 4 | s.type), 0x00});
    }
    const unsigned rec = 3 * s.width + (s.type == 1 ? 1 : 0), n = s.records * rec - s.cut;
    for (unsigned k = 0; k != n; ++k) {
      uint8_t b = mix(s.seed + k) & 0xFFU;
      if (s.type == 1 && k % rec == 0) {
        b &= 0x0FU;
      }
      m.push_back(b);
    }
  }
  if (f.message_bytes != ~0U) {
    m.resize(f.message_bytes);
  }
  const unsigned       size = 4 + m.size() + f.size_delta;
  std::vector<uint8_t> out(MAC_DST, MAC_DST + 6);
  out.insert(out.end(), MAC_SRC, MAC_SRC + 6);
  if (f.bad_dst) {
    out[5] ^= 1;
  }
  if (f.bad_src) {
    out[6] ^= 0x80;
  }
  out.insert(out.end(), {(uint8_t)(f.eth_type >> 8), (uint8_t)f.eth_type, (uint8_t)(f.revision << 4 | f.concatenation), (uint8_t)f.msg_type,
                         (uint8_t)(size >> 8), (uint8_t)size, (uint8_t)(f.eaxc >> 8), (uint8_t)f.eaxc, (uint8_t)f.seq, 0x80});
  out.insert(out.end(), m.begin(), m.end());
  if (out.size() < 64) {
    out.resize(64, 0);
  }
  if (f.length != 0) {
    out.resize(f.length);
  }
  return out;
}

// The frames of one batch.  Sequence identifiers count up per eAxC unless a frame says otherwise.
std::vector<frame_spec> frames_of(const config& c)
{
  std::vector<frame_spec> out;
  unsigned                next_seq[8] = {250, 250, 0, 0, 253, 250, 0, 0}; // eAxC 4 wraps 255 -> 0 early in the batch
  uint32_t                seed        = 1000;
  auto                    add         = [&](frame_spec f, const char* name, bool own_seq = false) {
    f.name = name;
    if (!own_seq) {
      f.seq = next_seq[f.eaxc & 7U]++ & 0xFFU;
    }
    for (section_spec& s : f.sections) {
      s.seed = seed;
      seed += 1000;
      if (c.static_compression) {
        s.type = c.type, s.width = c.width;
      }
    }
    out.push_back(f);
  };
  frame_spec base;
  auto       with = [&](auto change) {
    frame_spec f = base;
    change(f);
    return f;
  };
  add(base, "accepted");
  add(with([](frame_spec& f) { f.symbol = 4; }), "accepted, next symbol");
  add(with([](frame_spec& f) { f.symbol = 5; f.sections[0].type = 0; f.sections[0].width = 16; }), "accepted, none 16 when dynamic");
  add(with([](frame_spec& f) { f.symbol = 5; f.sections[0].start_prb = 3; f.sections[0].width = 14; }), "later frame over PRBs 3..5 of symbol 5");
  add(with([](frame_spec& f) { f.symbol = 6; }), "sequence wraps 255 -> 0 here or nearby");
  add(with([](frame_spec& f) { f.length = 60; }), "shorter than 64 bytes");
  add(with([](frame_spec& f) { f.bad_dst = true; }), "destination MAC");
  add(with([](frame_spec& f) { f.bad_src = true; }), "source MAC");
  add(with([](frame_spec& f) { f.eth_type = 0x0800; }), "Ethernet type");
  add(with([](frame_spec& f) { f.revision = 2; }), "eCPRI revision");
  add(with([](frame_spec& f) { f.concatenation = 1; }), "eCPRI concatenation");
  add(with([](frame_spec& f) { f.size_delta = 1; }), "payload size one more than the frame holds");
  add(with([](frame_spec& f) { f.size_delta = -1; }), "payload size one less: the section is incomplete when the size counts");
  add(with([](frame_spec& f) { f.msg_type = 2; }), "real-time control");
  add(with([](frame_spec& f) { f.msg_type = 5; }), "unknown eCPRI message type");
  add(with([](frame_spec& f) { f.eaxc = 9; }), "eAxC in neither list");
  add(with([](frame_spec& f) { f.subframe = 10; }), "subframe 10");
  add(with([](frame_spec& f) { f.slot = 2; }), "slot 2 at 30 kHz");
  add(with([](frame_spec& f) { f.message_bytes = 2; }), "message of 2 bytes");
  add(with([](frame_spec& f) { f.filter = 9; }), "reserved filter index");
  add(with([](frame_spec& f) { f.direction = 1; }), "downlink");
  add(with([](frame_spec& f) { f.version = 2; }), "payload version 2");
  add(with([](frame_spec& f) { f.symbol = 14; }), "symbol 14");
  if (!c.static_compression) {
    add(with([](frame_spec& f) { f.sections[0].type = 7; f.sections[0].records = 0; }), "reserved compression type 7");
    add(with([](frame_spec& f) { f.sections[0].type = 15; f.sections[0].records = 0; }), "reserved compression type 15");
    add(with([](frame_spec& f) { f.symbol = 7; f.sections[0].width = 1; }), "accepted, BFP 1");
    add(with([](frame_spec& f) { f.symbol = 8; f.sections[0].type = 0; f.sections[0].width = 2; }), "accepted, none 2");
  }
  add(with([](frame_spec& f) { f.sections.push_back(section_spec{5, 1, 1}); }), "two complete sections");
  add(with([](frame_spec& f) { f.message_bytes = 4; }), "header only: no section");
  add(with([](frame_spec& f) { f.sections[0].cut = 1; }), "records one byte short: no section");
  add(with([](frame_spec& f) { f.sections[0].nof_prbs_field = 4; }), "header claims one PRB more than sent: no section");
  add(with([](frame_spec& f) { f.symbol = 9; f.sections.push_back(section_spec{5, 1, 1}); f.sections[1].cut = 3; }),
      "one complete section and an incomplete one: accepted");
  add(with([](frame_spec& f) { f.symbol = 10; f.sections[0].nof_prbs_field = 1; f.sections[0].records = 1; }),
      "one PRB, padded to 64 bytes: accepted when the padding parses as an incomplete section");
  add(with([](frame_spec& f) { f.sfn8 = 9; }), "no expectation for the slot");
  add(with([](frame_spec& f) { f.eaxc = 5; f.symbol = 8; }), "symbol outside the announced range");
  add(with([](frame_spec& f) { f.subframe = 4; }), "announced with another filter index");
  add(with([](frame_spec& f) { f.eaxc = 0; }), "PRACH-only eAxC with filter index 0");
  add(with([](frame_spec& f) { f.sections[0].rb = 1; }), "every other RB");
  add(with([](frame_spec& f) { f.sections[0].sym_inc = 1; }), "symbol increment");
  add(with([](frame_spec& f) { f.eaxc = 5; f.sections[0].start_prb = 0; }), "starts below the announced PRBs");
  add(with([](frame_spec& f) { f.eaxc = 5; f.sections[0].start_prb = 6; }), "ends beyond the announced PRBs");
  add(with([](frame_spec& f) { f.slot = 0; f.symbol = 9; }), "no uplink context for the symbol");
  add(with([](frame_spec& f) { f.slot = 0; f.symbol = 6; }), "accepted into the second grid");
  add(with([](frame_spec& f) { f.symbol = 11; f.sections[0].nof_prbs_field = 0; f.sections[0].records = RU_PRBS; f.sections[0].start_prb = 5; }),
      "nof_prbs 0: all 9 PRBs from 0, clipped to the grid's 6");
  add(with([](frame_spec& f) { f.symbol = 12; f.sections[0].start_prb = 4; f.sections[0].nof_prbs_field = 4; f.sections[0].records = 4; }),
      "clipped: PRBs 4..7 of a 6-PRB grid");
  add(with([](frame_spec& f) { f.symbol = 12; f.sections[0].start_prb = 6; f.sections[0].nof_prbs_field = 2; f.sections[0].records = 2; }),
      "wholly beyond the grid: accepted, nothing written");
  add(with([](frame_spec& f) { f.eaxc = 0; f.filter = 1; }), "long PRACH");
  add(with([](frame_spec& f) { f.filter = 3; }), "short PRACH on a data eAxC");
  // the checker, on eAxC 5 (symbols 2..6, PRBs 1..7): first frame, in order, wrap, skipped ahead, from the past, in order again
  unsigned symbol = 2;
  for (unsigned seq : {254U, 255U, 0U, 3U, 2U, 250U, 4U, 132U, 131U}) {
    add(with([&](frame_spec& f) { f.eaxc = 5; f.seq = seq; f.symbol = 2 + symbol++ % 5; f.sections[0].start_prb = 1 + symbol % 4; }),
        "checker stream", true);
  }
  add(with([](frame_spec& f) { f.symbol = 13; f.seq = 100; }), "skipped ahead on eAxC 4", true);
  add(with([](frame_spec& f) { f.symbol = 13; f.seq = 99; f.sfn8 = 9; }), "from the past and no expectation: the checker drops it first", true);
  add(with([](frame_spec& f) { f.symbol = 13; f.seq = 101; f.direction = 1; }), "dropped after the checker: the state moves on", true);
  add(with([](frame_spec& f) { f.symbol = 13; f.seq = 102; }), "in order after a dropped frame", true);
  return out;
}

} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s OUT\n", argv[0]);
    return 1;
  }
  const std::string out_dir = argv[1];
  const config      configs[] = {{"payload size, static BFP 9", false, true, 1, 9},
                                 {"ignore size, static none 16", true, true, 0, 16},
                                 {"payload size, dynamic", false, false, 0, 0},
                                 {"ignore size, dynamic", true, false, 0, 0}};
  std::vector<uint8_t>  all_frames;
  std::vector<uint32_t> values;
  std::ostringstream    json;
  json << "{\n \"grid_nof_ports\": " << GRID_PORTS << ", \"grid_nof_subc\": " << GRID_SUBC << ", \"nof_grids\": 2,\n \"batches\": [\n";
  unsigned total = 0, written = 0;
  for (size_t ci = 0; ci != 4; ++ci) {
    const config& c = configs[ci];
    // what the control plane announced: (sfn8, subframe, slot, eaxc, filter, start_symbol, nof_symbols, prb_start, nof_prb, grid,
    // first and number of symbols with an uplink context)
    struct expectation {
      unsigned sfn8, subframe, slot, eaxc, filter, start_symbol, nof_symbols, prb_start, nof_prb, grid, ctx_start, ctx_len;
    };
    const expectation expects[] = {{7, 3, 1, 4, 0, 0, 14, 0, 9, 0, 0, 14},
                                   {7, 3, 1, 5, 0, 2, 5, 1, 7, 0, 0, 14},
                                   {7, 3, 0, 4, 0, 0, 14, 0, 9, 1, 0, 7},
                                   {7, 4, 1, 4, 1, 0, 14, 0, 9, 1, 0, 0}};
    auto        cplane_repo = std::make_shared<uplink_cplane_context_repository>(64);
    auto        ul_repo     = std::make_shared<uplink_context_repository>(64);
    grid_writer writers[2];
    resource_grid_dummy_with_spy_writer grid0(writers[0]), grid1(writers[1]);
    resource_grid*                      grids[2] = {&grid0, &grid1};
    for (const expectation& e : expects) {
      const slot_point  slot(1, e.sfn8, e.subframe, e.slot);
      ul_cplane_context context;
      context.prb_start              = e.prb_start;
      context.nof_prb                = e.nof_prb;
      context.nof_symbols            = e.nof_symbols;
      context.radio_hdr.start_symbol = e.start_symbol;
      context.radio_hdr.slot         = slot;
      context.radio_hdr.filter_index = to_filter_index_type(e.filter);
      context.radio_hdr.direction    = data_direction::uplink;
      cplane_repo->add(slot, e.eaxc, context);
      if (e.ctx_len != 0 && ul_repo->get(slot, e.ctx_start).empty()) {
        ul_repo->add({slot, 0}, *grids[e.grid], {e.ctx_start, e.ctx_start + e.ctx_len});
      }
    }
    rx_window_checker window_checker(logger(), {}, {});
    window_checker.on_new_symbol({{1, 0}, 0, 14});

    message_receiver_config rc;
    rc.nof_symbols = 14;
    rc.scs         = subcarrier_spacing::kHz30;
    std::memcpy(rc.vlan_params.mac_dst_address.data(), MAC_DST, 6);
    std::memcpy(rc.vlan_params.mac_src_address.data(), MAC_SRC, 6);
    rc.vlan_params.tci      = 4;
    rc.vlan_params.eth_type = ETH_TYPE;
    rc.ul_eaxc              = {4, 5};
    rc.prach_eaxc           = {0, 1};
    message_receiver_dependencies deps;
    deps.logger            = &logger();
    deps.window_checker    = &window_checker;
    deps.eth_receiver      = std::make_unique<eth_receiver_dummy>();
    deps.eth_frame_decoder = std::make_unique<vlan_decoder_wrap>();
    deps.ecpri_decoder     = std::make_unique<ecpri_decoder_wrap>(c.ignore_size);
    deps.seq_id_checker    = std::make_unique<checker_wrap>();
    deps.data_flow_prach   = std::make_unique<prach_flow_spy>();
    {
      std::unique_ptr<uplane_message_decoder> decoder;
      if (c.static_compression) {
        ru_compression_params params;
        params.type       = c.type == 0 ? compression_type::none : compression_type::BFP;
        params.data_width = c.width;
        decoder = std::make_unique<uplane_message_decoder_static_compression_impl>(logger(), subcarrier_spacing::kHz30, 14, RU_PRBS,
                                                                                   make_decompressor(), params);
      } else {
        decoder = std::make_unique<uplane_message_decoder_dynamic_compression_impl>(logger(), subcarrier_spacing::kHz30, 14, RU_PRBS,
                                                                                    make_decompressor());
      }
      data_flow_uplane_uplink_data_impl_config flow_config;
      flow_config.ul_eaxc = {4, 5};
      data_flow_uplane_uplink_data_impl_dependencies flow_deps;
      flow_deps.logger                 = &logger();
      flow_deps.notifier               = std::make_shared<notifier_spy>();
      flow_deps.ul_cplane_context_repo = cplane_repo;
      flow_deps.ul_context_repo        = ul_repo;
      flow_deps.uplane_decoder         = std::make_unique<uplane_decoder_wrap>(std::move(decoder));
      deps.data_flow_uplink =
          std::make_unique<data_flow_wrap>(std::make_unique<data_flow_uplane_uplink_data_impl>(flow_config, std::move(flow_deps)));
    }
    message_receiver_impl receiver(rc, std::move(deps));

    json << "  {\"name\": \"" << c.name << "\", \"ignore_ecpri_payload_size\": " << c.ignore_size
         << ", \"static_compression\": " << c.static_compression << ", \"type\": " << c.type << ", \"data_width\": " << c.width
         << ", \"ru_nof_prbs\": " << RU_PRBS << ", \"numerology\": 1, \"nof_symbols\": 14, \"ul_eaxc\": [4, 5], \"prach_eaxc\": [0, 1],\n"
         << "   \"expects\": [";
    for (size_t i = 0; i != 4; ++i) {
      const expectation& e    = expects[i];
      const unsigned     bits = e.ctx_len == 0 ? 0U : ((1U << e.ctx_len) - 1U) << e.ctx_start;
      json << (i ? ", " : "") << "{\"sfn8\": " << e.sfn8 << ", \"subframe\": " << e.subframe << ", \"slot\": " << e.slot
           << ", \"eaxc\": " << e.eaxc << ", \"filter_index\": " << e.filter << ", \"start_symbol\": " << e.start_symbol
           << ", \"nof_symbols\": " << e.nof_symbols << ", \"prb_start\": " << e.prb_start << ", \"nof_prb\": " << e.nof_prb
           << ", \"grid_index\": " << e.grid << ", \"context_symbols\": " << bits << "}";
    }
    json << "],\n   \"frames\": [\n";
    const std::vector<frame_spec> specs = frames_of(c);
    for (size_t fi = 0; fi != specs.size(); ++fi) {
      const std::vector<uint8_t> bytes = build(specs[fi], c);
      for (grid_writer& w : writers) {
        std::fill(w.store.begin(), w.store.end(), POISON);
      }
      now = trace{};
      receiver.on_new_frame(ether::unique_rx_buffer(rx_buffer_of(bytes)));
      if (now.notified) {
        std::fprintf(stderr, "%s / %s: a symbol was completed; the contexts changed\n", c.name, specs[fi].name.c_str());
        return 1;
      }
      // the one range this frame wrote, if any
      int      w_grid = -1;
      unsigned w_first = 0, w_count = 0;
      for (unsigned g = 0; g != 2; ++g) {
        for (unsigned k = 0; k != writers[g].store.size(); ++k) {
          if (writers[g].store[k] == POISON) {
            continue;
          }
          if (w_count != 0 && (w_grid != (int)g || k != w_first + w_count)) {
            std::fprintf(stderr, "%s / %s: the written elements are not one range\n", c.name, specs[fi].name.c_str());
            return 1;
          }
          if (w_count == 0) {
            w_grid = g, w_first = k;
          }
          ++w_count;
        }
      }
      json << "    {\"name\": \"" << specs[fi].name << "\", \"offset\": " << all_frames.size() << ", \"length\": " << bytes.size()
           << ", \"eth\": " << now.eth << ", \"ecpri\": " << now.ecpri << ", \"seq\": ";
      if (now.seq_asked) {
        json << now.seq;
      } else {
        json << "null";
      }
      json << ", \"flow\": " << now.flow << ", \"decoded\": " << now.decoded << ", \"write\": ";
      if (w_count == 0) {
        json << "null";
      } else {
        const unsigned row = w_first / GRID_SUBC;
        if ((w_first + w_count - 1) / GRID_SUBC != row) {
          std::fprintf(stderr, "%s / %s: a write crosses a symbol\n", c.name, specs[fi].name.c_str());
          return 1;
        }
        json << "{\"grid\": " << w_grid << ", \"port\": " << row / 14 << ", \"symbol\": " << row % 14 << ", \"first_subc\": " << w_first % GRID_SUBC
             << ", \"nof_subc\": " << w_count << ", \"values_offset\": " << values.size() << "}";
        for (unsigned k = w_first; k != w_first + w_count; ++k) {
          uint32_t w;
          std::memcpy(&w, &writers[w_grid].store[k], 4);
          values.push_back(w);
        }
        ++written;
      }
      json << "}" << (fi + 1 != specs.size() ? "," : "") << "\n";
      all_frames.insert(all_frames.end(), bytes.begin(), bytes.end());
      ++total;
    }
    json << "   ]}" << (ci + 1 != 4 ? "," : "") << "\n";
  }
  json << " ]\n}\n";
  std::ofstream(out_dir + "/ofh_rx_reference_cases.json") << json.str();
  write_npy(out_dir + "/ofh_rx_reference_frames.npy", "|u1", all_frames);
  write_npy(out_dir + "/ofh_rx_reference_values.npy", "<u4", values);
  std::printf("%u frames, %u of them wrote, %zu bytes, %zu words\n", total, written, all_frames.size(), values.size());
  return 0;
}
