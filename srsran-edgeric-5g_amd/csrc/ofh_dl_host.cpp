// Host side of the Open Fronthaul downlink transmit (ofh_dl_kernels.hip): the reference's fragmentation of a symbol, validation
// of flows and descriptors, the header of a symbol's first frame, and the per-symbol records one launch reads.
#include "nrphy_host_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace nrphy;

namespace {

constexpr uint32_t ETH_ECPRI_HEADER = 18 + 8; // vlan_frame_builder_impl + ecpri::packet_builder_impl (iq_data)
constexpr uint32_t MIN_FRAME = 64, MAX_FRAME = 9600; // MIN_ETH_FRAME_LENGTH, MAX_ETH_FRAME_LENGTH

struct Layout {
  uint32_t header_bytes, record_bytes, prbs_per_frag, nof_frags;
  uint32_t prbs(uint32_t f, uint32_t ru_nof_prbs) const { return std::min(prbs_per_frag, ru_nof_prbs - f * prbs_per_frag); }
  uint32_t frame_bytes(uint32_t f, uint32_t ru_nof_prbs) const { return std::max(MIN_FRAME, header_bytes + prbs(f, ru_nof_prbs) * record_bytes); }
};

// ofh_uplane_fragment_size_calculator(0, ru_nof_prbs, compr).calculate_fragment_size(..., mtu - headers) until it says last.
bool flow_layout(const nrphy_ofh_dl_flow_t& f, Layout* out)
{
  const nrphy_ofh_compression_cfg_t& c = f.compression;
  if (c.type > 1 || c.data_width < 8 || c.data_width > 16 || !std::isfinite(c.iq_scaling) || f.ru_nof_prbs == 0 ||
      f.ru_nof_prbs > NRPHY_MAX_RB || f.static_compression > 1 || f.mtu > MAX_FRAME || f.mtu < MIN_FRAME) {
    return false;
  }
  Layout l;
  l.header_bytes = ETH_ECPRI_HEADER + (f.static_compression ? 8U : 10U);
  l.record_bytes = 3U * c.data_width + c.type;
  if (f.mtu < l.header_bytes + l.record_bytes) {
    return false;
  }
  l.prbs_per_frag = std::min((f.mtu - l.header_bytes) / l.record_bytes, f.ru_nof_prbs);
  l.nof_frags     = (f.ru_nof_prbs + l.prbs_per_frag - 1) / l.prbs_per_frag;
  *out            = l;
  return true;
}

struct Range {
  uint64_t first, last;
  bool     operator<(const Range& o) const { return first < o.first; }
};

// Validation and, with `items`, the records of the launch (frame addresses are d_frames + offsets: `frames_address` gives
// their alignment, which decides how a frame is cut into windows).
int dl_items(uint32_t n_flows, const nrphy_ofh_dl_flow_t* flows, uint32_t n, const nrphy_ofh_dl_symbol_t* symbols, uint32_t nof_grids,
             uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint64_t frames_bytes, uint32_t frame_stride, uintptr_t frames_address,
             std::vector<OfhDlSymbol>* items, uint32_t* nof_wgs)
{
  if ((n_flows != 0 && flows == nullptr) || (n != 0 && symbols == nullptr) || grid_nof_subc % 12U != 0 || frame_stride % 16U != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Layout> layouts(n_flows);
  for (uint32_t i = 0; i != n_flows; ++i) {
    if (!flow_layout(flows[i], &layouts[i])) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  std::vector<Range> ranges;
  ranges.reserve(n_flows == 1 ? (size_t)n * layouts[0].nof_frags : n);
  if (items != nullptr) {
    items->reserve(n);
  }
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_ofh_dl_symbol_t& s = symbols[i];
    if (s.flow >= n_flows || s.grid_index >= nof_grids || s.port >= grid_nof_ports || s.symbol >= NRPHY_NSYMB || s.subframe >= 10 ||
        s.slot >= 16 || s.sfn >= 1024 || s.reserved_[0] != 0 || s.reserved_[1] != 0) {
      return NRPHY_ERR_ARGUMENT;
    }
    const nrphy_ofh_dl_flow_t& f = flows[s.flow];
    const Layout&              l = layouts[s.flow];
    if (grid_nof_subc > 12U * f.ru_nof_prbs || frame_stride < f.mtu) {
      return NRPHY_ERR_ARGUMENT;
    }
    // Every fragment but the last is at most mtu <= frame_stride bytes long: when the last one ends inside the buffer, all do.
    const uint64_t last_at = (uint64_t)(l.nof_frags - 1) * frame_stride, last_bytes = l.frame_bytes(l.nof_frags - 1, f.ru_nof_prbs);
    if (s.frame_offset > frames_bytes || last_at > frames_bytes - s.frame_offset || last_bytes > frames_bytes - s.frame_offset - last_at) {
      return NRPHY_ERR_ARGUMENT;
    }
    const uint64_t full_bytes = l.frame_bytes(0, f.ru_nof_prbs);
    for (uint32_t k = 0; k + 1 < l.nof_frags; ++k) {
      const uint64_t first = s.frame_offset + (uint64_t)k * frame_stride;
      ranges.push_back({first, first + full_bytes});
    }
    ranges.push_back({s.frame_offset + last_at, s.frame_offset + last_at + last_bytes});
    if (items == nullptr) {
      continue;
    }
    OfhDlSymbol it;
    std::memset(&it, 0, sizeof it);
    it.frame         = s.frame_offset;
    it.row           = (((uint64_t)s.grid_index * grid_nof_ports + s.port) * NRPHY_NSYMB + s.symbol) * grid_nof_subc;
    it.first_wg      = *nof_wgs;
    it.stride        = frame_stride;
    it.window        = (62U * l.record_bytes / 16U) * 16U; // at most 64 records have a byte in it
    it.nof_frags     = (uint16_t)l.nof_frags;
    it.prbs_per_frag = (uint16_t)l.prbs_per_frag;
    it.nof_prbs      = (uint16_t)f.ru_nof_prbs;
    it.grid_prbs     = (uint16_t)(grid_nof_subc / 12U);
    it.data_width    = (uint8_t)f.compression.data_width;
    it.bfp           = (uint8_t)f.compression.type;
    // the AVX2 compressors convert the whole call at once for BFP and for the widths their packer has (9, 16)
    it.whole_span   = (f.compression.type == 1 || f.compression.data_width == 9 || f.compression.data_width == 16) ? 1 : 0;
    it.header_bytes = (uint8_t)l.header_bytes;
    // quantizer: gain = 2^(width - 1) - 1, 16 bits for BFP (Q_BIT_WIDTH); scale = gain * iq_scaling in float
    const float gain = (float)((1 << ((f.compression.type == 1 ? 16 : (int)f.compression.data_width) - 1)) - 1.0F);
    it.scale         = gain * f.compression.iq_scaling;
    uint8_t* h       = it.header;
    std::memcpy(h, f.mac_dst, 6);
    std::memcpy(h + 6, f.mac_src, 6);
    h[12] = 0x81, h[13] = 0x00; // VLAN_TPID
    h[14] = (uint8_t)(f.tci >> 8), h[15] = (uint8_t)f.tci;
    h[16] = (uint8_t)(f.eth_type >> 8), h[17] = (uint8_t)f.eth_type;
    h[18] = 0x10; // eCPRI revision 1, no concatenation
    h[19] = 0x00; // message_type::iq_data
    // 20, 21: payload size, per fragment
    h[22] = (uint8_t)(s.eaxc >> 8), h[23] = (uint8_t)s.eaxc;
    h[24] = s.seq_id; // + fragment
    h[25] = 0x80;     // E bit, subsequence 0
    h[26] = 0x90;     // downlink, payload version 1, filter index 0
    h[27] = (uint8_t)s.sfn;
    h[28] = (uint8_t)(s.subframe << 4 | s.slot >> 2);
    h[29] = (uint8_t)((s.slot & 3U) << 6 | s.symbol);
    // 30: section identifier 0; 31 ... 33: start and number of PRBs, per fragment
    h[34] = (uint8_t)(f.compression.data_width << 4 | f.compression.type); // dynamic builder only, as is byte 35 = 0
    // Windows of the frames: all fragments of a symbol have the same address modulo 16 (frame_stride is a multiple of 16).
    const uint32_t mis  = (uint32_t)((frames_address + s.frame_offset) & 15U);
    const auto     wins = [&](uint32_t k) { return (l.frame_bytes(k, f.ru_nof_prbs) + mis + it.window - 1) / it.window; };
    it.windows_per_frag = wins(0);
    *nof_wgs += (l.nof_frags - 1) * it.windows_per_frag + wins(l.nof_frags - 1);
    items->push_back(it);
  }
  if (!std::is_sorted(ranges.begin(), ranges.end())) { // descriptors usually come in the order of their frames
    std::sort(ranges.begin(), ranges.end());
  }
  for (size_t i = 1; i < ranges.size(); ++i) {
    if (ranges[i].first < ranges[i - 1].last) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ofh_dl_fragments(const nrphy_ofh_dl_flow_t* flow, uint32_t max, nrphy_ofh_dl_fragment_t* out, uint32_t* n)
{
  Layout l;
  if (flow == nullptr || n == nullptr || !flow_layout(*flow, &l)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *n = l.nof_frags;
  if (max < l.nof_frags || out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t k = 0; k != l.nof_frags; ++k) {
    out[k].start_prb   = (uint16_t)(k * l.prbs_per_frag);
    out[k].nof_prbs    = (uint16_t)l.prbs(k, flow->ru_nof_prbs);
    out[k].frame_bytes = l.frame_bytes(k, flow->ru_nof_prbs);
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_dl_validate(uint32_t n_flows, const nrphy_ofh_dl_flow_t* flows, uint32_t n, const nrphy_ofh_dl_symbol_t* symbols,
                                     uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint64_t frames_bytes,
                                     uint32_t frame_stride)
{
  return dl_items(n_flows, flows, n, symbols, nof_grids, grid_nof_ports, grid_nof_subc, frames_bytes, frame_stride, 0, nullptr, nullptr);
}

extern "C" int nrphy_ofh_dl_write_frames(nrphy_ctx_t* ctx, uint32_t n_flows, const nrphy_ofh_dl_flow_t* flows, uint32_t n,
                                         const nrphy_ofh_dl_symbol_t* symbols, const void* d_grid, uint32_t nof_grids,
                                         uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint8_t* d_frames, uint64_t frames_bytes,
                                         uint32_t frame_stride, void* stream)
{
  if (ctx == nullptr || (reinterpret_cast<uintptr_t>(d_grid) & 15U) != 0 || (reinterpret_cast<uintptr_t>(d_frames) & 15U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<OfhDlSymbol> items;
  uint32_t                 nof_wgs = 0;
  const int rc = dl_items(n_flows, flows, n, symbols, nof_grids, grid_nof_ports, grid_nof_subc, frames_bytes, frame_stride,
                          reinterpret_cast<uintptr_t>(d_frames), &items, &nof_wgs);
  if (rc != NRPHY_OK) {
    return rc;
  }
  if (items.empty()) {
    return NRPHY_OK;
  }
  if (d_grid == nullptr || d_frames == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t   s = stream ? (hipStream_t)stream : ctx->stream;
  StreamStaging staging(s);
  OfhDlSymbol*  d_items = (OfhDlSymbol*)staging.alloc(items.size() * sizeof(OfhDlSymbol));
  if (d_items == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(OfhDlSymbol), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_ofh_dl_frames(d_items, (uint32_t)items.size(), nof_wgs, (const uint32_t*)d_grid, d_frames, s));
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_dl_frames_host(nrphy_ctx_t* ctx, const nrphy_ofh_dl_flow_t* flow, const nrphy_ofh_dl_symbol_t* symbol,
                                        const void* row, uint32_t grid_nof_subc, uint8_t* frames, uint64_t frames_bytes,
                                        uint32_t frame_stride)
{
  if (ctx == nullptr || flow == nullptr || symbol == nullptr || row == nullptr || frames == nullptr || symbol->flow != 0 ||
      symbol->grid_index != 0 || symbol->port != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  // Declared before the HostCall: the launch's records are read by an asynchronous copy.
  std::vector<OfhDlSymbol> items;
  uint32_t                 nof_wgs = 0;
  // The device copy of `frames` sits 256-byte aligned at the same offsets, so the windows are those of an aligned buffer.
  const int rc = dl_items(1, flow, 1, symbol, 1, 1, grid_nof_subc, frames_bytes, frame_stride, 0, &items, &nof_wgs);
  if (rc != NRPHY_OK) {
    return rc;
  }
  Layout l;
  flow_layout(*flow, &l);
  // The one row as symbol 0 of a grid of its own; of the frames only the span the symbol's fragments cover is staged.
  items[0].row = 0;
  const uint64_t span_first = symbol->frame_offset & ~(uint64_t)15;
  const uint64_t span_bytes = symbol->frame_offset - span_first + (uint64_t)(l.nof_frags - 1) * frame_stride +
                              l.frame_bytes(l.nof_frags - 1, flow->ru_nof_prbs);
  items[0].frame = symbol->frame_offset - span_first;
  HostCall     call(ctx);
  const size_t row_bytes = std::max<size_t>(4 * (size_t)grid_nof_subc, 16);
  uint8_t*     piece[3];
  if (!call.carve(SCRATCH_GRID, {row_bytes, sizeof(OfhDlSymbol), (size_t)span_bytes}, piece)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(piece[0], row, 4 * (size_t)grid_nof_subc, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(piece[1], items.data(), sizeof(OfhDlSymbol), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(launch_ofh_dl_frames((const OfhDlSymbol*)piece[1], 1, nof_wgs, (const uint32_t*)piece[0], piece[2], ctx->stream));
  for (uint32_t k = 0; k != l.nof_frags; ++k) {
    const uint64_t at = (uint64_t)k * frame_stride;
    HIP_TRY(hipMemcpyAsync(frames + symbol->frame_offset + at, piece[2] + items[0].frame + at, l.frame_bytes(k, flow->ru_nof_prbs),
                           hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(call.sync());
  return NRPHY_OK;
}
