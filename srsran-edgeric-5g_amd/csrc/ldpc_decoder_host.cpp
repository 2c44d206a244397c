// Host side of ldpc_decoder.hip: the decoder's graphs and early-stop tables (built on first use, kept by the context), its
// scratch layout and its launch; and the per-codeblock host form that runs rate dematcher and decoder in one round trip.
#include "ldpc_base_graph_host.h"
#include "ldpc_receive_host.h"
#include "nrphy_trace.h"

#include <cmath>

namespace {

// Decoder graph of (base graph, lifting size): all edges of TS 38.212 Tables 5.3.2-2/-3, row by row.
const DecoderGraph* get_decoder_graph(nrphy_ctx* ctx, unsigned bg, unsigned zc)
{
  const int pos = lifting_position(zc);
  if (pos < 0) {
    return nullptr;
  }
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  const unsigned slot = (bg - 1) * NOF_LIFTING_SIZES + (unsigned)pos;
  if (ctx->d_dec_graph[slot] == nullptr) {
    std::vector<DecoderGraph> g(1);
    std::memset(&g[0], 0, sizeof(DecoderGraph));
    const nr_ldpc_edge_t* edges   = (bg == 1) ? NR_LDPC_BG1_EDGES : NR_LDPC_BG2_EDGES;
    const unsigned        n_edges = (bg == 1) ? NR_LDPC_BG1_NOF_EDGES : NR_LDPC_BG2_NOF_EDGES;
    const unsigned        rows    = (bg == 1) ? 46 : 42;
    const int             ils     = lifting_set_index(zc);
    unsigned              count   = 0;
    for (unsigned m = 0; m != rows; ++m) {
      g[0].row_ptr[m] = count;
      for (unsigned e = 0; e != n_edges; ++e) {
        if (edges[e].row == m) {
          g[0].edge[count++] = (((uint32_t)edges[e].col * zc) << 16) | (edges[e].shift[ils] % zc); // 67 * 384 < 2^16
        }
      }
    }
    for (unsigned m = rows; m != MAX_BG_ROWS + 2; ++m) {
      g[0].row_ptr[m] = count;
    }
    for (unsigned m = 0, pairs = 0; m != MAX_BG_ROWS + 2; ++m) {
      g[0].pair_ptr[m] = pairs;
      pairs += m + 1 < MAX_BG_ROWS + 2 ? (g[0].row_ptr[m + 1] - g[0].row_ptr[m] + 1) / 2 : 0;
    }
    for (unsigned m = 0; m != rows; ++m) {
      // the kernel is specialised for the row degrees the two base graphs have
      const unsigned deg = g[0].row_ptr[m + 1] - g[0].row_ptr[m];
      if (!((deg >= 3 && deg <= 10) || deg == 19)) {
        return nullptr;
      }
    }
    for (unsigned m = 0, quads = 0; m != MAX_BG_ROWS + 2; ++m) {
      g[0].quad_ptr[m] = quads;
      quads += m + 1 < MAX_BG_ROWS + 2 ? (g[0].row_ptr[m + 1] - g[0].row_ptr[m] + 3) / 4 : 0;
    }
    if ((zc & 1U) == 0) {
      // Two checks per lane with the messages in LDS: where lane j finds the soft bits of checks j and j + Zc / 2 on every edge
      // -- (variable node * Zc + (check + shift) mod Zc), the first in the low half of a word, the second in the high half --
      // as [row of four edges][lane][edge in the row]: the same for every codeblock and iteration, so the kernel reads the
      // words of a layer (sixteen bytes per lane and row, a layer ahead) instead of computing them (7 vector instructions per
      // edge and pass).  Five spare rows: the kernel always reads five rows from a layer's first.
      const unsigned        half = zc / 2, total = g[0].quad_ptr[rows] + 5;
      std::vector<uint32_t> addr((size_t)total * half * 4, 0);
      for (unsigned m = 0; m != rows; ++m) {
        const unsigned e0 = g[0].row_ptr[m], deg = g[0].row_ptr[m + 1] - e0;
        for (unsigned t = 0; t != deg; ++t) {
          const unsigned base = g[0].edge[e0 + t] >> 16, shift = g[0].edge[e0 + t] & 0xFFFFU;
          for (unsigned j = 0; j != half; ++j) {
            const unsigned a1 = base + (j + shift) % zc, a2 = base + (j + half + shift) % zc; // < 68 * 384 < 2^16
            addr[((size_t)(g[0].quad_ptr[m] + t / 4) * half + j) * 4 + t % 4] = a1 | (a2 << 16);
          }
        }
      }
      if (upload(&ctx->d_dec_addr[slot], addr.data(), addr.size() * sizeof(uint32_t)) != hipSuccess) {
        return nullptr;
      }
    }
    if (upload(&ctx->d_dec_graph[slot], g.data(), sizeof(DecoderGraph)) != hipSuccess) {
      return nullptr;
    }
  }
  return ctx->d_dec_graph[slot];
}

const uint32_t* get_decoder_pair_addresses(nrphy_ctx* ctx, unsigned bg, unsigned zc)
{
  const int pos = lifting_position(zc);
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  return pos < 0 ? nullptr : ctx->d_dec_addr[(bg - 1) * NOF_LIFTING_SIZES + (unsigned)pos];
}

// Early-stop tables: word w of the n-bit message (32 bits, the last one n mod 32) is followed by n - 32 w - bits(w)
// bits; the message is a multiple of the generator g iff the sum of word(w) * x^(that) vanishes mod g.  Per word eight
// nibble tables, tab[w][k][v] = (v x^(4 k)) * x^(bits after word w) mod g: the product is eight independent look-ups
// instead of a 32-step shift-and-add per word and iteration (which was about 15 % of an early-stop iteration).
const uint32_t* get_decoder_crc_weights(nrphy_ctx* ctx, uint32_t poly, uint32_t order, uint32_t n_msg)
{
  const uint64_t key = ((uint64_t)poly << 32) | n_msg;
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  auto           it  = ctx->d_dec_crc.find(key);
  if (it != ctx->d_dec_crc.end()) {
    return it->second;
  }
  const CrcField        field = {poly, order};
  const uint32_t        nw    = (n_msg + 31) / 32;
  std::vector<uint32_t> w((size_t)nw * DEC_CRC_TABLE_WORDS);
  for (uint32_t i = 0; i != nw; ++i) {
    const uint32_t bits   = std::min<uint32_t>(32, n_msg - 32 * i);
    const uint32_t weight = field.xpow((int64_t)n_msg - 32 * i - bits);
    for (uint32_t k = 0; k != 8; ++k) {
      for (uint32_t v = 0; v != 16; ++v) {
        w[(size_t)i * DEC_CRC_TABLE_WORDS + 16 * k + v] = field.mul(weight, v << (4 * k));
      }
    }
  }
  uint32_t* d = nullptr;
  if (upload(&d, w.data(), w.size() * sizeof(uint32_t)) != hipSuccess) {
    return nullptr;
  }
  ctx->d_dec_crc[key] = d;
  return d;
}

// What every entry point of the decoder asks of a configuration: base graph 1 or 2 at one of the 51 lifting sizes.
bool decoder_graph_valid(const nrphy_ldpc_decoder_cfg_t& cfg)
{
  return (cfg.base_graph == 1 || cfg.base_graph == 2) && lifting_position(cfg.lifting_size) >= 0;
}
unsigned decoder_bg_k(const nrphy_ldpc_decoder_cfg_t& cfg) { return (cfg.base_graph == 1) ? 22 : 10; } // message nodes
// cfg.crc_poly (0: no early stop, 16, 0x24A, 0x24B) -> generator polynomial and order; false: none of these.
bool decoder_crc(uint32_t id, uint32_t& poly, uint32_t& order)
{
  poly  = id == 16 ? 0x11021U : id == 0x24A ? 0x1864CFBU : id == 0x24B ? 0x1800063U : 0;
  order = poly == 0 ? 0 : id == 16 ? 16 : 24;
  return id == 0 || poly != 0;
}
// Rows of two edges that the messages per edge of a base graph's first `layers` layers take (ldpc_decoder.hip): the sum of
// ceil(degree / 2).
uint32_t decoder_message_rows(unsigned base_graph, uint32_t layers)
{
  const nr_ldpc_edge_t* edges   = (base_graph == 1) ? NR_LDPC_BG1_EDGES : NR_LDPC_BG2_EDGES;
  const unsigned        n_edges = (base_graph == 1) ? NR_LDPC_BG1_NOF_EDGES : NR_LDPC_BG2_NOF_EDGES;
  std::vector<uint32_t> degree(layers, 0);
  for (unsigned e = 0; e != n_edges; ++e) {
    if (edges[e].row < layers) {
      ++degree[edges[e].row];
    }
  }
  uint32_t rows = 0;
  for (uint32_t dg : degree) {
    rows += (dg + 1) / 2;
  }
  return rows;
}

// The caller-owned scratch of a decoder launch: a pool of slots (check records or messages per edge) + their flags.
struct DecoderScratch {
  uint32_t nof_slots, nof_layers_max;
  uint64_t slot_bytes, records_bytes, flags_bytes, total_bytes;
};
bool decoder_scratch_layout(const nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t& cfg, uint32_t n_cb, DecoderScratch& s)
{
  if (!decoder_graph_valid(cfg) || n_cb == 0) {
    return false;
  }
  const unsigned bg_k = decoder_bg_k(cfg), zc = cfg.lifting_size;
  const uint32_t nof_nodes = std::max<uint32_t>(divide_ceil(cfg.nof_llr, zc) + 2, bg_k + 4);
  s.nof_layers_max         = nof_nodes - bg_k;
  // Workgroups of the decoder the device can hold at once: 32 wavefronts per CU (the kernel is built for 8 per SIMD),
  // ceil(Zc / 64) per workgroup; one slot per CU more as a margin.  A smaller batch gets a slot per codeblock.
  const uint32_t waves    = divide_ceil(zc, 64);
  const uint32_t resident = ctx->nof_cus * (32U / waves) + ctx->nof_cus;
  s.nof_slots             = std::min<uint32_t>(n_cb, resident);
  if (ctx->tune.decoder_slots_all) { // profiling aid (profiles/): a slot per codeblock, i.e. no pooling
    s.nof_slots = n_cb;
  }
  // A slot holds a codeblock's check records (8 bytes per lifted check and layer) or, with two checks per lane, its messages
  // per edge: rows of two edges, 2 Zc bytes each, five spare rows (the kernel requests five rows from a layer's first).
  const uint64_t rows     = 5 + (uint64_t)decoder_message_rows(cfg.base_graph, s.nof_layers_max);
  s.slot_bytes            = (std::max<uint64_t>((uint64_t)s.nof_layers_max * zc * sizeof(uint2), rows * 2 * zc) + 255) & ~(uint64_t)255;
  s.records_bytes         = (uint64_t)s.nof_slots * s.slot_bytes;
  s.flags_bytes           = ((uint64_t)s.nof_slots * 4 + 255) & ~(uint64_t)255;
  s.total_bytes           = ((s.records_bytes + 255) & ~(uint64_t)255) + s.flags_bytes;
  return true;
}
} // namespace

extern "C" int nrphy_ldpc_decoder_scratch_bytes(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb,
                                                uint64_t* bytes)
{
  DecoderScratch s;
  if (ctx == nullptr || cfg == nullptr || bytes == nullptr || !decoder_scratch_layout(ctx, *cfg, n_cb, s)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *bytes = s.total_bytes;
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_decoder_prepare(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg)
{
  uint32_t poly, order;
  if (ctx == nullptr || cfg == nullptr || !decoder_graph_valid(*cfg) || !decoder_crc(cfg->crc_poly, poly, order)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (get_decoder_graph(ctx, cfg->base_graph, cfg->lifting_size) == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  if (order != 0) {
    const uint32_t K = decoder_bg_k(*cfg) * cfg->lifting_size;
    if (cfg->nof_filler_bits >= K || get_decoder_crc_weights(ctx, poly, order, K - cfg->nof_filler_bits) == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_decode(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb,
                                 const int8_t* d_llr, uint32_t llr_stride_bytes, uint8_t* d_out,
                                 uint32_t out_stride_bytes, uint32_t* d_iterations, void* d_scratch, void* stream)
{
  return ldpc_decode_batch(ctx, cfg, n_cb, d_llr, llr_stride_bytes, d_out, out_stride_bytes, d_iterations, nullptr,
                           nullptr, false, d_scratch, stream);
}

int ldpc_decode_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb, const int8_t* d_llr,
                      uint32_t llr_stride_bytes, uint8_t* d_out, uint32_t out_stride_bytes, uint32_t* d_iterations,
                      const uint8_t* d_skip, uint8_t* d_ok_flags, bool crc_at_end, void* d_scratch, void* stream,
                      uint32_t expected_extent)
{
  LdpcDecodeLaunch p;
  if (ctx == nullptr || cfg == nullptr || d_llr == nullptr || d_out == nullptr || d_scratch == nullptr ||
      !decoder_graph_valid(*cfg) || cfg->max_iterations == 0 ||
      !(cfg->scaling_factor > 0.0F && cfg->scaling_factor < 1.0F) || !decoder_crc(cfg->crc_poly, p.crc_poly, p.crc_order)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned bg_k = decoder_bg_k(*cfg), n_full = (cfg->base_graph == 1) ? 68 : 52;
  const unsigned zc = cfg->lifting_size, K = bg_k * zc;
  // ldpc_decoder_impl.cpp:70-86: between the message plus two blocks and the whole (shortened) codeblock.
  if (cfg->nof_llr < K + 2 * zc || cfg->nof_llr > (n_full - 2) * zc ||
      cfg->nof_filler_bits >= K || llr_stride_bytes < cfg->nof_llr || out_stride_bytes < (K + 7) / 8) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  p.graph     = get_decoder_graph(ctx, cfg->base_graph, zc);
  p.pair_addr = get_decoder_pair_addresses(ctx, cfg->base_graph, zc);
  if (p.graph == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  p.zc             = zc;
  p.bg_k           = bg_k;
  p.nof_nodes      = std::max<uint32_t>(divide_ceil(cfg->nof_llr, zc) + 2, bg_k + 4);
  p.nof_layers_max = p.nof_nodes - bg_k;
  p.nof_llr        = cfg->nof_llr;
  p.llr_stride     = llr_stride_bytes;
  p.out_stride     = out_stride_bytes;
  p.nof_filler     = cfg->nof_filler_bits;
  p.max_iterations = cfg->max_iterations;
  p.scaling_factor = cfg->scaling_factor;
  p.llr            = d_llr;
  p.out            = d_out;
  p.iterations     = d_iterations;
  p.skip           = d_skip;
  p.ok_flags       = d_ok_flags;
  p.crc_at_end     = crc_at_end ? 1U : 0U;
  p.knob_pairs     = ctx->tune.decoder_pairs;
  p.knob_ldsmsg    = ctx->tune.decoder_ldsmsg;
  {
    // LDS for the messages-per-edge form (ldpc_decoder.hip) at the expected extent: the soft bits of the layers it needs (the
    // kernel's own rule: ldpc_decoder_impl.cpp:88-116), then one byte per edge and lifted check of those layers.
    const uint32_t extent = (expected_extent == 0 || expected_extent > cfg->nof_llr) ? cfg->nof_llr : expected_extent;
    uint32_t       cb_len = std::max<uint32_t>(extent + 2 * zc, K + 4 * zc);
    cb_len                = divide_ceil(cb_len, zc) * zc;
    p.lm_lds_bytes        = ((cb_len + 48U + 15U) & ~15U) + decoder_message_rows(cfg->base_graph, cb_len / zc - bg_k) * 2 * zc;
    // The scaling of the minima by arithmetic instead of a table look-up, where it gives the table's values
    // (round half away from zero: ldpc_decoder_generic.cpp:69-79).
    p.scale_arithmetic = 1;
    p.scale_fixed      = (uint32_t)std::lround((double)cfg->scaling_factor * 512.0); // < 512: 120 * F + 256 stays below 2^16
    bool fixed_ok      = p.scale_fixed < 512;
    for (unsigned m = 0; m <= 120; ++m) {
      const float    x    = (float)m * cfg->scaling_factor;
      const uint32_t want = (uint32_t)(uint8_t)roundf(x);
      if ((uint32_t)(x + 0.5F) != want) {
        p.scale_arithmetic = 0;
      }
      if (((m * p.scale_fixed + 256U) & 0xFFFFU) >> 9 != want) {
        fixed_ok = false;
      }
    }
    if (fixed_ok) {
      p.scale_arithmetic = 2;
    }
  }
  p.crc_weight     = nullptr;
  if (p.crc_order != 0) {
    // Uploaded by nrphy_ldpc_decoder_prepare(); a first use without it allocates and copies here (not capturable).
    p.crc_weight = get_decoder_crc_weights(ctx, p.crc_poly, p.crc_order, K - cfg->nof_filler_bits);
    if (p.crc_weight == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  if (n_cb == 0) {
    return NRPHY_OK;
  }
  // Check records or messages per edge: the caller's scratch, a pool of slots shared by the workgroups resident at once.
  DecoderScratch sl;
  if (!decoder_scratch_layout(ctx, *cfg, n_cb, sl)) {
    return NRPHY_ERR_ARGUMENT;
  }
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  p.scratch     = (uint2*)d_scratch;
  p.slot_flags = (uint32_t*)((uint8_t*)d_scratch + ((sl.records_bytes + 255) & ~(uint64_t)255));
  p.nof_slots   = sl.nof_slots;
  p.slot_bytes  = (uint32_t)sl.slot_bytes;
  if (sl.nof_slots < n_cb) {
    HIP_TRY(hipMemsetAsync(p.slot_flags, 0, sl.flags_bytes, s));
  }
  {
    const TraceRange trace("cb_decode");
    HIP_TRY(launch_ldpc_decode(p, n_cb, s));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_decode_host(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, const int8_t* llr,
                                      uint8_t* message_packed, uint32_t* iterations)
{
  if (ctx == nullptr || cfg == nullptr || llr == nullptr || message_packed == nullptr || !decoder_graph_valid(*cfg) ||
      cfg->nof_llr > 66U * cfg->lifting_size) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned K     = decoder_bg_k(*cfg) * cfg->lifting_size;
  HostCall       call(ctx);
  uint8_t*       d[2]; // soft bits; message, then the iteration count at the next multiple of 4
  if (!call.carve(SCRATCH_RX, {(size_t)cfg->nof_llr + 16, (size_t)(K + 7) / 8 + 16}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  int8_t*   d_llr = (int8_t*)d[0];
  uint8_t*  d_out = d[1];
  uint32_t* d_it  = (uint32_t*)(d_out + (((K + 7) / 8 + 3) & ~3U));
  HIP_TRY(hipMemcpy(d_llr, llr, cfg->nof_llr, hipMemcpyHostToDevice));
  uint64_t scratch_bytes = 0;
  if (nrphy_ldpc_decoder_scratch_bytes(ctx, cfg, 1, &scratch_bytes) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  void* d_scratch = call.mem(SCRATCH_DECODER, scratch_bytes);
  if (d_scratch == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  const int rc = nrphy_ldpc_decode(ctx, cfg, 1, d_llr, cfg->nof_llr, d_out, (K + 7) / 8, d_it, d_scratch, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  uint32_t it = 0;
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(message_packed, d_out, (K + 7) / 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&it, d_it, sizeof(it), hipMemcpyDeviceToHost));
  if (iterations) {
    *iterations = it;
  }
  return NRPHY_OK;
}

// One codeblock through rate dematcher and decoder with one round trip over the link: what a per-codeblock
// accelerator interface (hal::hw_accelerator_pusch_dec) asks for.
extern "C" int nrphy_pusch_decode_codeblock_host(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* dm,
                                                 uint32_t crc_poly, uint32_t max_iterations, float scaling_factor,
                                                 const int8_t* llr, int8_t* soft_buffer, int new_data,
                                                 uint8_t* message_packed, uint32_t* iterations)
{
  if (ctx == nullptr || dm == nullptr || llr == nullptr || soft_buffer == nullptr || message_packed == nullptr ||
      (dm->base_graph != 1 && dm->base_graph != 2) || lifting_position(dm->lifting_size) < 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned zc = dm->lifting_size, n = ((dm->base_graph == 1) ? 66U : 50U) * zc;
  const unsigned k = ((dm->base_graph == 1) ? 22U : 10U) * zc, kbytes = (k + 7) / 8;
  const size_t   off_soft = ((size_t)dm->rm_length + 63) & ~(size_t)63, off_out = off_soft + (((size_t)n + 63) & ~(size_t)63);
  const size_t   off_it = off_out + (((size_t)kbytes + 63) & ~(size_t)63);
  HostCall call(ctx);
  uint8_t* base = call.mem<uint8_t>(SCRATCH_RX, off_it + 64);
  if (base == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(base, llr, dm->rm_length, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(base + off_soft, soft_buffer, n, hipMemcpyHostToDevice, ctx->stream));
  int rc = nrphy_ldpc_rate_dematch(ctx, dm, 1, (const int8_t*)base, dm->rm_length, (int8_t*)(base + off_soft), n, new_data,
                                   ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  nrphy_ldpc_decoder_cfg_t dec;
  dec.base_graph      = dm->base_graph;
  dec.lifting_size    = zc;
  dec.nof_filler_bits = dm->nof_filler_bits;
  dec.crc_poly        = crc_poly;
  dec.nof_llr         = n;
  dec.max_iterations  = max_iterations;
  dec.scaling_factor  = scaling_factor;
  uint64_t scratch_bytes = 0;
  if (nrphy_ldpc_decoder_scratch_bytes(ctx, &dec, 1, &scratch_bytes) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  void* d_scratch = call.mem(SCRATCH_DECODER, scratch_bytes);
  if (d_scratch == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  rc = nrphy_ldpc_decode(ctx, &dec, 1, (const int8_t*)(base + off_soft), n, base + off_out, kbytes,
                         (uint32_t*)(base + off_it), d_scratch, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  uint32_t it = 0;
  HIP_TRY(hipMemcpyAsync(soft_buffer, base + off_soft, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(message_packed, base + off_out, kbytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(&it, base + off_it, sizeof(it), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  if (iterations) {
    *iterations = it;
  }
  return NRPHY_OK;
}
