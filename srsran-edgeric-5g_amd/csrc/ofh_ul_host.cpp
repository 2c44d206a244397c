// Host side of the Open Fronthaul uplink receive (ofh_ul_kernels.hip): validation of the section lists, the range arithmetic
// of the reference's two data-flow writers, and the item list one launch reads.
#include "nrphy_host_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace nrphy;

namespace {

bool compression_ok(uint32_t type, uint32_t width)
{
  // none with 1 bit has a quantiser gain of 0: the reference divides by it
  return type <= 1 && width <= 16 && width >= (type == 1 ? 1U : 2U);
}

// What every section must satisfy whatever it is written to: udCompHdr, PRB count, the padding, and all of its records as
// sent inside the payload (check_iq_data_size, ofh_uplane_message_decoder_impl.cpp).
bool section_ok(const nrphy_ofh_ul_section_t& s, uint64_t payload_bytes)
{
  if (!compression_ok(s.type, s.data_width) || s.nof_prbs == 0 || s.nof_prbs > NRPHY_MAX_RB || s.reserved_ != 0) {
    return false;
  }
  const uint64_t bytes = (uint64_t)s.nof_prbs * (3U * s.data_width + s.type);
  return s.payload_offset <= payload_bytes && bytes <= payload_bytes - s.payload_offset;
}

struct Range {
  uint64_t first, last; // destination elements [first, last)
  bool     operator<(const Range& o) const { return first < o.first; }
};

bool disjoint(std::vector<Range>& ranges)
{
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i) {
    if (ranges[i].first < ranges[i - 1].last) {
      return false;
    }
  }
  return true;
}

void add_item(std::vector<OfhUlItem>& items, uint32_t& nof_chunks, const nrphy_ofh_ul_section_t& s, uint32_t first_re, uint32_t nof_re,
              uint64_t dst)
{
  OfhUlItem it;
  it.src         = s.payload_offset + (uint64_t)(first_re / 12U) * (3U * s.data_width + s.type);
  it.dst         = dst;
  it.nof_re      = nof_re;
  it.re_skip     = first_re % 12U;
  it.first_chunk = nof_chunks;
  it.data_width  = s.data_width;
  it.bfp         = s.type;
  items.push_back(it);
  nof_chunks += ((it.re_skip + nof_re + 11U) / 12U + OFH_UL_PRBS_PER_WG - 1) / OFH_UL_PRBS_PER_WG;
}

// uplane_rx_symbol_data_flow_writer::write_to_resource_grid (ofh_uplane_rx_symbol_data_flow_writer.cpp:53-80) per section;
// `items` may be null (validation only).
int grid_items(uint32_t n, const nrphy_ofh_ul_section_t* sections, uint64_t payload_bytes, uint32_t nof_grids, uint32_t grid_nof_ports,
               uint32_t grid_nof_subc, std::vector<OfhUlItem>* items, uint32_t* nof_chunks)
{
  if ((n != 0 && sections == nullptr) || grid_nof_subc % 12U != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t     du_nof_prbs = grid_nof_subc / 12U;
  std::vector<Range> ranges;
  ranges.reserve(n);
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_ofh_ul_section_t& s = sections[i];
    if (!section_ok(s, payload_bytes) || s.symbol >= NRPHY_NSYMB || s.port >= grid_nof_ports || s.grid_index >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    if (s.start_prb >= du_nof_prbs) {
      continue;
    }
    uint32_t nof_prbs_to_write = du_nof_prbs - s.start_prb;
    if ((uint32_t)s.start_prb + s.nof_prbs < du_nof_prbs) {
      nof_prbs_to_write = s.nof_prbs;
    }
    const uint64_t dst = (((uint64_t)s.grid_index * grid_nof_ports + s.port) * NRPHY_NSYMB + s.symbol) * grid_nof_subc + 12U * s.start_prb;
    ranges.push_back({dst, dst + 12U * nof_prbs_to_write});
    if (items != nullptr) {
      add_item(*items, *nof_chunks, s, 0, 12U * nof_prbs_to_write, dst);
    }
  }
  return disjoint(ranges) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

// uplane_prach_symbol_data_flow_writer::write_to_prach_buffer (ofh_uplane_prach_symbol_data_flow_writer.cpp:56-112) per
// section, in its order and with its integer types.
int prach_items(uint32_t n, const nrphy_ofh_ul_prach_section_t* sections, uint64_t payload_bytes, uint64_t symbols_elems,
                std::vector<OfhUlItem>* items, uint32_t* nof_chunks)
{
  if (n != 0 && sections == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Range> ranges;
  ranges.reserve(n);
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_ofh_ul_prach_section_t& ps = sections[i];
    const nrphy_ofh_ul_section_t&       s  = ps.section;
    if (!section_ok(s, payload_bytes) || s.grid_index != 0 || s.port != 0 || s.symbol != 0 ||
        (ps.prach_nof_re != 139 && ps.prach_nof_re != 839)) {
      return NRPHY_ERR_ARGUMENT;
    }
    const unsigned section_start_prb = s.start_prb, section_nof_prbs = s.nof_prbs;
    const unsigned prach_nof_res = ps.prach_nof_re, nof_re_to_prach_data = ps.offset_to_first_re;
    const unsigned prach_nof_prbs          = (unsigned)std::ceil(float(prach_nof_res + nof_re_to_prach_data) / 12);
    const unsigned nof_re_after_prach_data = prach_nof_prbs * 12U - (prach_nof_res + nof_re_to_prach_data);
    const unsigned prach_data_start_prb    = nof_re_to_prach_data / 12U;
    if (section_start_prb >= prach_nof_prbs || section_start_prb + section_nof_prbs <= prach_data_start_prb) {
      continue;
    }
    unsigned nof_prbs_to_write = prach_nof_prbs - section_start_prb;
    if (section_start_prb + section_nof_prbs < prach_nof_prbs) {
      nof_prbs_to_write = section_nof_prbs;
    }
    const unsigned start_re         = (unsigned)std::max<int>(0, (int)(section_start_prb * 12U - nof_re_to_prach_data));
    const unsigned section_start_re = section_start_prb * 12U;
    unsigned       section_nof_re   = nof_prbs_to_write * 12U;
    if (section_start_prb + section_nof_prbs >= prach_nof_prbs) {
      section_nof_re -= nof_re_after_prach_data;
    }
    unsigned iq_start_re = 0;
    if (section_start_re < nof_re_to_prach_data) {
      iq_start_re = nof_re_to_prach_data - section_start_re;
      section_nof_re -= iq_start_re;
    }
    const unsigned iq_size_re = std::min(section_nof_re, prach_nof_res);
    // the reference's subspan of the section's samples: inside them, or its assertion fires
    if ((uint64_t)iq_start_re + iq_size_re > 12U * section_nof_prbs) {
      return NRPHY_ERR_ARGUMENT;
    }
    if (iq_size_re == 0) {
      continue;
    }
    if (ps.dst_offset > symbols_elems || (uint64_t)start_re + iq_size_re > symbols_elems - ps.dst_offset) {
      return NRPHY_ERR_ARGUMENT;
    }
    const uint64_t dst = ps.dst_offset + start_re;
    ranges.push_back({dst, dst + iq_size_re});
    if (items != nullptr) {
      add_item(*items, *nof_chunks, s, iq_start_re, iq_size_re, dst);
    }
  }
  return disjoint(ranges) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

// Copies the items into staging that lives in stream order for this call, and launches.
int run_items(nrphy_ctx* ctx, const std::vector<OfhUlItem>& items, uint32_t nof_chunks, const uint8_t* d_payload, void* d_dst, bool prach,
              void* stream)
{
  if (items.empty()) {
    return NRPHY_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t   s = stream ? (hipStream_t)stream : ctx->stream;
  StreamStaging staging(s);
  OfhUlItem*    d_items = (OfhUlItem*)staging.alloc(items.size() * sizeof(OfhUlItem));
  if (d_items == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(OfhUlItem), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_ofh_ul_sections(d_items, (uint32_t)items.size(), nof_chunks, d_payload, d_dst, prach, s));
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ofh_decompress(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t n_rows, uint32_t nof_prb,
                                    const uint8_t* d_in, size_t in_row_stride, void* d_prbs, size_t row_stride, void* stream)
{
  if (ctx == nullptr || cfg == nullptr || d_in == nullptr || d_prbs == nullptr || !compression_ok(cfg->type, cfg->data_width) ||
      nof_prb > NRPHY_MAX_RB || (reinterpret_cast<uintptr_t>(d_prbs) & 3U) != 0 ||
      (n_rows > 1 && (row_stride < 12 * (size_t)nof_prb || in_row_stride < (size_t)nof_prb * nrphy_ofh_compressed_prb_bytes(cfg)))) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  for (uint32_t first = 0; first < n_rows; first += 32768) {
    OfhDecompressLaunch p;
    p.in            = d_in + first * in_row_stride;
    p.prbs          = (uint32_t*)d_prbs + first * row_stride;
    p.in_row_stride = in_row_stride;
    p.row_stride    = row_stride;
    p.nof_prb       = nof_prb;
    p.data_width    = cfg->data_width;
    p.bfp           = cfg->type;
    HIP_TRY(launch_ofh_decompress(p, std::min<uint32_t>(32768, n_rows - first), s));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_decompress_host(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t nof_prb, const uint8_t* in,
                                         void* prbs)
{
  if (ctx == nullptr || cfg == nullptr || in == nullptr || prbs == nullptr || nof_prb == 0 || nof_prb > NRPHY_MAX_RB ||
      !compression_ok(cfg->type, cfg->data_width)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall     call(ctx);
  const size_t in_bytes = (size_t)nof_prb * nrphy_ofh_compressed_prb_bytes(cfg), out_bytes = (size_t)nof_prb * 48;
  uint8_t*     piece[2];
  if (!call.carve(SCRATCH_GRID, {in_bytes, out_bytes}, piece)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(piece[0], in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_ofh_decompress(ctx, cfg, 1, nof_prb, piece[0], in_bytes, piece[1], 12 * (size_t)nof_prb, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(prbs, piece[1], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_ul_validate(uint32_t n, const nrphy_ofh_ul_section_t* sections, uint64_t payload_bytes, uint32_t nof_grids,
                                     uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return grid_items(n, sections, payload_bytes, nof_grids, grid_nof_ports, grid_nof_subc, nullptr, nullptr);
}

extern "C" int nrphy_ofh_ul_write_grid(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ofh_ul_section_t* sections, const uint8_t* d_payload,
                                       uint64_t payload_bytes, void* d_grid, uint32_t nof_grids, uint32_t grid_nof_ports,
                                       uint32_t grid_nof_subc, void* stream)
{
  if (ctx == nullptr || (reinterpret_cast<uintptr_t>(d_grid) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<OfhUlItem> items;
  uint32_t               nof_chunks = 0;
  const int rc = grid_items(n, sections, payload_bytes, nof_grids, grid_nof_ports, grid_nof_subc, &items, &nof_chunks);
  if (rc != NRPHY_OK) {
    return rc;
  }
  if (!items.empty() && (d_payload == nullptr || d_grid == nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  return run_items(ctx, items, nof_chunks, d_payload, d_grid, false, stream);
}

extern "C" int nrphy_ofh_ul_prach_validate(uint32_t n, const nrphy_ofh_ul_prach_section_t* sections, uint64_t payload_bytes,
                                           uint64_t symbols_elems)
{
  return prach_items(n, sections, payload_bytes, symbols_elems, nullptr, nullptr);
}

extern "C" int nrphy_ofh_ul_write_prach(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ofh_ul_prach_section_t* sections, const uint8_t* d_payload,
                                        uint64_t payload_bytes, void* d_symbols, uint64_t symbols_elems, void* stream)
{
  if (ctx == nullptr || (reinterpret_cast<uintptr_t>(d_symbols) & 7U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<OfhUlItem> items;
  uint32_t               nof_chunks = 0;
  const int              rc         = prach_items(n, sections, payload_bytes, symbols_elems, &items, &nof_chunks);
  if (rc != NRPHY_OK) {
    return rc;
  }
  if (!items.empty() && (d_payload == nullptr || d_symbols == nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  return run_items(ctx, items, nof_chunks, d_payload, d_symbols, true, stream);
}
