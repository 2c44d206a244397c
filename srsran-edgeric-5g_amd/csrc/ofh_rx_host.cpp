// Host side of the Open Fronthaul uplink frame receiver (ofh_rx_kernels.hip): validation of the configuration, of the frame
// ranges and of the expectations, the object that owns the checker state and the ownership table, and the staging of a call.
#include "nrphy_host_internal.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace nrphy;

struct nrphy_ofh_rx {
  nrphy_ctx*         ctx       = nullptr;
  nrphy_ofh_rx_cfg_t cfg       = {};
  uint32_t*          d_state   = nullptr; // OFH_RX_MAX_EAXC words
  uint32_t*          d_own     = nullptr; // grown to the largest grid batch seen
  size_t             own_words = 0;
};

namespace {

constexpr uint32_t MAX_EAXC_VALUE = 32; // MAX_SUPPORTED_EAXC_ID_VALUE

bool compression_ok(const nrphy_ofh_compression_cfg_t& c)
{
  return c.type <= 1 && c.data_width <= 16 && c.data_width >= (c.type == 1 ? 1U : 2U); // what nrphy_ofh_decompress takes
}

bool eaxc_list_ok(uint32_t n, const uint16_t* list)
{
  if (n > 4) {
    return false;
  }
  for (uint32_t i = 0; i != n; ++i) {
    if (list[i] >= MAX_EAXC_VALUE || std::find(list, list + i, list[i]) != list + i) {
      return false;
    }
  }
  return true;
}

bool cfg_ok(const nrphy_ofh_rx_cfg_t& c)
{
  return c.reserved_ == 0 && c.vlan_tag_present <= 1 && c.ignore_ecpri_payload_size <= 1 && c.seq_id_check <= 1 && c.numerology <= 4 &&
         (c.nof_symbols == 14 || c.nof_symbols == 12) && c.ru_nof_prbs >= 1 && c.ru_nof_prbs <= NRPHY_MAX_RB && c.static_compression <= 1 &&
         eaxc_list_ok(c.n_ul_eaxc, c.ul_eaxc) && eaxc_list_ok(c.n_prach_eaxc, c.prach_eaxc) &&
         (c.static_compression == 0 || (compression_ok(c.compression) && compression_ok(c.prach_compression)));
}

struct Range {
  uint64_t first, last;
  bool     operator<(const Range& o) const { return first < o.first; }
};

int validate(const nrphy_ofh_rx_cfg_t* cfg, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect,
             const nrphy_ofh_rx_expect_t* expects, uint64_t frames_bytes, uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  if (cfg == nullptr || !cfg_ok(*cfg) || (n_frames != 0 && frames == nullptr) || (n_expect != 0 && expects == nullptr) ||
      grid_nof_subc % 12U != 0 || cfg->n_ul_eaxc > grid_nof_ports) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Range> ranges;
  ranges.reserve(n_frames);
  for (uint32_t i = 0; i != n_frames; ++i) {
    const nrphy_ofh_rx_frame_t& f = frames[i];
    if (f.reserved_ != 0 || f.offset > frames_bytes || f.length > frames_bytes - f.offset) {
      return NRPHY_ERR_ARGUMENT;
    }
    if (f.length != 0) {
      ranges.push_back({f.offset, f.offset + f.length});
    }
  }
  if (!std::is_sorted(ranges.begin(), ranges.end())) { // frames usually come in the order of their bytes
    std::sort(ranges.begin(), ranges.end());
  }
  for (size_t i = 1; i < ranges.size(); ++i) {
    if (ranges[i].first < ranges[i - 1].last) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  std::vector<uint64_t> keys;
  keys.reserve(n_expect);
  for (uint32_t i = 0; i != n_expect; ++i) {
    const nrphy_ofh_rx_expect_t& e = expects[i];
    if (std::find(cfg->ul_eaxc, cfg->ul_eaxc + cfg->n_ul_eaxc, e.eaxc) == cfg->ul_eaxc + cfg->n_ul_eaxc || e.grid_index >= nof_grids ||
        e.sfn8 >= 256 || e.subframe >= 10 || e.slot >= (1U << cfg->numerology) || e.filter_index > 7 || e.reserved_ != 0 ||
        (uint32_t)e.start_symbol + e.nof_symbols > cfg->nof_symbols || (uint32_t)e.prb_start + e.nof_prb > NRPHY_MAX_RB) {
      return NRPHY_ERR_ARGUMENT;
    }
    keys.push_back((uint64_t)e.sfn8 << 32 | (uint64_t)e.subframe << 24 | (uint64_t)e.slot << 16 | e.eaxc);
  }
  std::sort(keys.begin(), keys.end());
  return std::adjacent_find(keys.begin(), keys.end()) == keys.end() ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

// Write-pass workgroups per frame, from the frame lengths alone: no frame holds more PRB records than its bytes after the
// shortest headers allow, no section more than 275, and none is written beyond the grid.
uint32_t chunks_per_frame(const nrphy_ofh_rx_cfg_t& c, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t grid_nof_subc)
{
  uint32_t max_length = 0;
  for (uint32_t i = 0; i != n_frames; ++i) {
    max_length = std::max(max_length, frames[i].length);
  }
  const uint32_t headers = (c.vlan_tag_present ? 18U : 14U) + 8U + 4U + 4U + (c.static_compression ? 0U : 2U);
  // dynamic: BFP with 1 bit is the smallest record the write pass takes
  const uint32_t record = c.static_compression ? 3U * c.compression.data_width + c.compression.type : 4U;
  const uint32_t prbs   = max_length > headers ? (max_length - headers) / record : 0U;
  return (std::min({prbs, (uint32_t)NRPHY_MAX_RB, grid_nof_subc / 12U}) + OFH_UL_PRBS_PER_WG - 1) / OFH_UL_PRBS_PER_WG;
}

int run(nrphy_ofh_rx* rx, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect, const nrphy_ofh_rx_expect_t* expects,
        const uint8_t* d_frames, uint64_t frames_bytes, void* d_grid, uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
        nrphy_ofh_rx_record_t* d_records, hipStream_t s)
{
  const nrphy_ofh_rx_cfg_t& c = rx->cfg;
  const int rc = validate(&c, n_frames, frames, n_expect, expects, frames_bytes, nof_grids, grid_nof_ports, grid_nof_subc);
  if (rc != NRPHY_OK || n_frames == 0) {
    return rc;
  }
  if (d_frames == nullptr || d_grid == nullptr || d_records == nullptr || (reinterpret_cast<uintptr_t>(d_grid) & 3U) != 0 ||
      (reinterpret_cast<uintptr_t>(d_records) & 7U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t own_words = (size_t)nof_grids * grid_nof_ports * NRPHY_NSYMB * (grid_nof_subc / 12U);
  if (own_words > UINT32_MAX) { // the kernels index the table with 32 bits
    return NRPHY_ERR_ARGUMENT;
  }
  if (own_words > rx->own_words) { // growth waits for the device: a launch in flight may still read the old table
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(rx->d_own);
    rx->d_own     = nullptr;
    rx->own_words = 0;
    HIP_TRY(hipMalloc((void**)&rx->d_own, own_words * sizeof(uint32_t)));
    rx->own_words = own_words;
  }
  // one staging buffer: the frames, then the expectations (16-byte entries in front of 4-byte aligned ones)
  const size_t         frames_size = (size_t)n_frames * sizeof(nrphy_ofh_rx_frame_t), expects_size = (size_t)n_expect * sizeof(nrphy_ofh_rx_expect_t);
  std::vector<uint8_t> host(frames_size + expects_size);
  std::memcpy(host.data(), frames, frames_size);
  if (n_expect != 0) {
    std::memcpy(host.data() + frames_size, expects, expects_size);
  }
  StreamStaging staging(s);
  uint8_t*      d_host = (uint8_t*)staging.alloc(host.size());
  if (d_host == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(d_host, host.data(), host.size(), hipMemcpyHostToDevice, s));
  if (own_words != 0) {
    HIP_TRY(hipMemsetAsync(rx->d_own, 0, own_words * sizeof(uint32_t), s));
  }
  OfhRxLaunch p;
  std::memset(&p, 0, sizeof p);
  p.frames             = (const nrphy_ofh_rx_frame_t*)d_host;
  p.expects            = (const nrphy_ofh_rx_expect_t*)(d_host + frames_size);
  p.d_frames           = d_frames;
  p.records            = d_records;
  p.grid               = (uint32_t*)d_grid;
  p.state              = rx->d_state;
  p.own                = rx->d_own;
  p.n_frames           = n_frames;
  p.n_expect           = n_expect;
  p.grid_nof_ports     = grid_nof_ports;
  p.grid_nof_subc      = grid_nof_subc;
  p.chunks_per_frame   = chunks_per_frame(c, n_frames, frames, grid_nof_subc);
  p.eth_header         = c.vlan_tag_present ? 18U : 14U;
  p.eth_type           = c.eth_type;
  p.ignore_size        = c.ignore_ecpri_payload_size;
  p.seq_id_check       = c.seq_id_check;
  p.numerology         = c.numerology;
  p.nof_symbols        = c.nof_symbols;
  p.ru_nof_prbs        = c.ru_nof_prbs;
  p.static_compression = c.static_compression;
  p.n_ul_eaxc          = c.n_ul_eaxc;
  p.n_prach_eaxc       = c.n_prach_eaxc;
  // one checker lane per distinct eAxC value: an eAxC in both lists has one counter, as in the reference
  for (uint32_t k = 0; k != c.n_ul_eaxc + c.n_prach_eaxc; ++k) {
    const uint16_t v = k < c.n_ul_eaxc ? c.ul_eaxc[k] : c.prach_eaxc[k - c.n_ul_eaxc];
    if (std::find(p.eaxc, p.eaxc + p.n_eaxc, v) == p.eaxc + p.n_eaxc) {
      p.eaxc[p.n_eaxc++] = v;
    }
  }
  std::memcpy(p.ul_eaxc, c.ul_eaxc, sizeof p.ul_eaxc);
  std::memcpy(p.prach_eaxc, c.prach_eaxc, sizeof p.prach_eaxc);
  std::memcpy(p.mac, c.mac_dst, 6);
  std::memcpy(p.mac + 6, c.mac_src, 6);
  p.type[0]       = (uint8_t)c.compression.type;
  p.type[1]       = (uint8_t)c.prach_compression.type;
  p.data_width[0] = (uint8_t)c.compression.data_width;
  p.data_width[1] = (uint8_t)c.prach_compression.data_width;
  HIP_TRY(launch_ofh_rx(p, s));
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ofh_rx_validate(const nrphy_ofh_rx_cfg_t* cfg, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect,
                                     const nrphy_ofh_rx_expect_t* expects, uint64_t frames_bytes, uint32_t nof_grids,
                                     uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, n_frames, frames, n_expect, expects, frames_bytes, nof_grids, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_ofh_rx_destroy(nrphy_ofh_rx_t* rx)
{
  if (rx == nullptr) {
    return NRPHY_OK;
  }
  (void)hipSetDevice(rx->ctx->device);
  (void)hipFree(rx->d_state); // waits for the device: no launch of this object is in flight afterwards
  (void)hipFree(rx->d_own);
  delete rx;
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_rx_create(nrphy_ctx_t* ctx, const nrphy_ofh_rx_cfg_t* cfg, nrphy_ofh_rx_t** out)
{
  if (out != nullptr) {
    *out = nullptr;
  }
  if (ctx == nullptr || cfg == nullptr || out == nullptr || !cfg_ok(*cfg)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  auto* rx = new nrphy_ofh_rx;
  rx->ctx  = ctx;
  rx->cfg  = *cfg;
  if (hipMalloc((void**)&rx->d_state, OFH_RX_MAX_EAXC * sizeof(uint32_t)) != hipSuccess ||
      hipMemsetAsync(rx->d_state, 0, OFH_RX_MAX_EAXC * sizeof(uint32_t), ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    nrphy_ofh_rx_destroy(rx);
    return NRPHY_ERR_DEVICE;
  }
  *out = rx;
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_rx_reset(nrphy_ofh_rx_t* rx, void* stream)
{
  if (rx == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(rx->ctx->device));
  HIP_TRY(hipMemsetAsync(rx->d_state, 0, OFH_RX_MAX_EAXC * sizeof(uint32_t), stream ? (hipStream_t)stream : rx->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_rx_run(nrphy_ofh_rx_t* rx, uint32_t n_frames, const nrphy_ofh_rx_frame_t* frames, uint32_t n_expect,
                                const nrphy_ofh_rx_expect_t* expects, const uint8_t* d_frames, uint64_t frames_bytes, void* d_grid,
                                uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_ofh_rx_record_t* d_records,
                                void* stream)
{
  if (rx == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(rx->ctx->device));
  return run(rx, n_frames, frames, n_expect, expects, d_frames, frames_bytes, d_grid, nof_grids, grid_nof_ports, grid_nof_subc, d_records,
             stream ? (hipStream_t)stream : rx->ctx->stream);
}

extern "C" int nrphy_ofh_rx_host(nrphy_ofh_rx_t* rx, const uint8_t* frame, uint32_t length, uint32_t n_expect,
                                 const nrphy_ofh_rx_expect_t* expects, void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                 nrphy_ofh_rx_record_t* record)
{
  if (rx == nullptr || frame == nullptr || length == 0 || grid == nullptr || record == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_ofh_rx_frame_t desc = {0, length, 0};
  const int rc = validate(&rx->cfg, 1, &desc, n_expect, expects, length, 1, grid_nof_ports, grid_nof_subc);
  if (rc != NRPHY_OK) {
    return rc;
  }
  nrphy_ctx*   ctx = rx->ctx;
  HostCall     call(ctx);
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  uint8_t*     piece[3];
  if (!call.carve(SCRATCH_GRID, {(size_t)length, std::max<size_t>(grid_bytes, 16), sizeof(nrphy_ofh_rx_record_t)}, piece)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(piece[0], frame, length, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(piece[1], grid, grid_bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc_run = run(rx, 1, &desc, n_expect, expects, piece[0], length, piece[1], 1, grid_nof_ports, grid_nof_subc,
                         (nrphy_ofh_rx_record_t*)piece[2], ctx->stream);
  if (rc_run != NRPHY_OK) {
    return rc_run;
  }
  HIP_TRY(hipMemcpyAsync(grid, piece[1], grid_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(record, piece[2], sizeof(nrphy_ofh_rx_record_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}
