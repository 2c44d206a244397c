// Host side of libmi355nrphy.so: the C ABI of include/mi355_nrphy.h.
//
// The context and its tables, the OFDM plan, the LDPC encoder, dematcher and decoders and the PUSCH decoder: plan construction
// and kernel launches (the PDSCH plan lives in pdsch_plan_build.cpp and pdsch_host.cpp).  No compute happens here and there is
// no CPU fallback: every entry point that produces PHY output needs a HIP device.
#include "pdsch_plan.h"
#include "nrphy_trace.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <array>
#include <map>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

using namespace nrphy;

namespace {

struct nr_ldpc_edge_t {
  uint8_t  row;
  uint8_t  col;
  uint16_t shift[8];
};
#include "nr_ldpc_bg.inc"

// Lifting-set index i_LS: Zc = a * 2^j, a in {2, 3, 5, 7, 9, 11, 13, 15} (TS 38.212 Table 5.3.2-1).
int lifting_set_index(unsigned zc)
{
  static const unsigned base[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  for (int i = 0; i != 8; ++i) {
    for (unsigned v = base[i]; v <= 384; v *= 2) {
      if (v == zc) {
        return i;
      }
    }
  }
  return -1;
}

} // namespace

void build_lifted_graph(unsigned bg, unsigned zc, LiftedGraph& g)
{
  const nr_ldpc_edge_t* edges   = (bg == 1) ? NR_LDPC_BG1_EDGES : NR_LDPC_BG2_EDGES;
  const unsigned        n_edges = (bg == 1) ? NR_LDPC_BG1_NOF_EDGES : NR_LDPC_BG2_NOF_EDGES;
  const unsigned        kb      = (bg == 1) ? 22 : 10;
  const unsigned        rows    = (bg == 1) ? 46 : 42;
  const int             ils     = lifting_set_index(zc);
  std::memset(&g, 0, sizeof(g));
  int      core_shift[4] = {-1, -1, -1, -1};
  unsigned count         = 0;
  for (unsigned m = 0; m != rows; ++m) {
    g.row_ptr[m] = (uint16_t)count;
    for (unsigned e = 0; e != n_edges; ++e) {
      if (edges[e].row != m) {
        continue;
      }
      unsigned col = edges[e].col, shift = edges[e].shift[ils] % zc;
      if (m < 4) {
        if (col == kb) {
          core_shift[m] = (int)shift;
        }
        if (col >= kb) {
          continue; // core rows: systematic part only, the parity part is solved in closed form
        }
      } else if (col >= kb + 4) {
        continue; // the identity column of an extension row is its own parity block
      }
      if (m < 4 && (zc & 31U) == 0) {
        // Core rows of word-aligned lifting sizes read a doubled copy of the systematic blocks (ldpc_device.h,
        // core_row_word_dbl): byte offset of word q' of the doubled block, and the funnel shift s'.
        const unsigned wpb = zc / 32, sh = shift & 31U, q = shift >> 5;
        const unsigned qd = (sh != 0) ? q : (q + wpb - 1) % wpb, sd = (32U - sh) & 31U;
        g.edge[count++] = ((4U * (2U * wpb * col + qd)) << 16) | sd;
        continue;
      }
      g.edge[count++] = ((col * zc) << 16) | shift; // bit offset of the block in the codeblock (< 2^16), lifted shift
    }
  }
  for (unsigned m = rows; m != MAX_BG_ROWS + 2; ++m) {
    g.row_ptr[m] = (uint16_t)count;
  }
  unsigned mid = (core_shift[1] >= 0) ? 1 : 2;
  int      s0 = core_shift[0], s3 = core_shift[3], sm = core_shift[mid];
  g.core_mid = (uint16_t)mid;
  g.core_s0  = (uint16_t)s0;
  g.core_s3  = (uint16_t)s3;
  g.core_b   = (uint16_t)((s0 == s3) ? sm : ((s0 == sm) ? s3 : s0));
}

namespace {

// ---- Gold sequence tables (TS 38.211 Section 5.2.1) -----------------------------------------------------------
// 31x31 matrices over GF(2) as 31 row masks.
void mat_mul(const uint32_t* a, const uint32_t* b, uint32_t* out) // out = a * b
{
  uint32_t bt[31];                      // columns of b
  for (int c = 0; c != 31; ++c) {
    uint32_t col = 0;
    for (int r = 0; r != 31; ++r) {
      col |= ((b[r] >> c) & 1U) << r;
    }
    bt[c] = col;
  }
  uint32_t tmp[31];
  for (int r = 0; r != 31; ++r) {
    uint32_t row = 0;
    for (int c = 0; c != 31; ++c) {
      row |= (uint32_t)(__builtin_popcount(a[r] & bt[c]) & 1) << c;
    }
    tmp[r] = row;
  }
  std::memcpy(out, tmp, sizeof(tmp));
}

// GF(2)[x] / g arithmetic of the transport-block CRC polynomials (order 24 or 16, `poly` with its leading term).

void build_tbcrc_tables(TbCrcTables& t)
{
  const CrcField* field[2] = {&CRC24A_FIELD, &CRC16_FIELD};
  for (unsigned s = 0; s != 2; ++s) {
    const CrcField& f  = *field[s];
    const uint32_t  y32 = f.xpow(32), y1k = f.xpow(32 * 1024), y8k = f.xpow(128 * 64), yz = f.xpow(8 * (int64_t)TB_CRC_REGION_BYTES);
    for (unsigned k = 0; k != 4; ++k) {
      for (uint32_t b = 0; b != 256; ++b) {
        t.y32[s][k][b] = f.mul(y32, b << (8 * k));
        t.y1k[s][k][b] = f.mul(y1k, b << (8 * k));
        t.y8k[s][k][b] = f.mul(y8k, b << (8 * k));
        t.yz[s][k][b]  = f.mul(yz, b << (8 * k));
      }
    }
    for (unsigned l = 0; l != 64; ++l) {
      t.lane[s][l] = f.xpow(128 * (63 - (int)l));
    }
  }
}

void build_gold_tables(GoldTables& t, std::vector<uint32_t>& x1_words)
{
  std::memset(&t, 0, sizeof(t));
  // One step of x2: state'[j] = state[j+1], state'[30] = state[3]^state[2]^state[1]^state[0].
  uint32_t m[31];
  for (int r = 0; r != 30; ++r) {
    m[r] = 1U << (r + 1);
  }
  m[30] = 0xF;
  for (int k = 0; k != GOLD_JUMP_BITS; ++k) {
    std::memcpy(t.x2_jump[k], m, sizeof(m));
    mat_mul(m, m, m);
  }
  // The next 992 bits are linear in the state: x2_head[t][w] is the state mask of bit 32 w + t.
  for (int i = 0; i != 31; ++i) {
    uint32_t st = 1U << i;
    for (int n = 0; n != 992; ++n) {
      if (st & 1U) {
        t.x2_head[n & 31][n >> 5] |= 1U << i;
      }
      uint32_t f = ((st >> 3) ^ (st >> 2) ^ (st >> 1) ^ st) & 1U;
      st         = (st >> 1) | (f << 30);
    }
  }
  // x^(32 m) mod CRC24B and the CRC24B byte table.
  const uint32_t poly = 0x1800063U, top = 1U << 24;
  uint32_t       v    = 1;
  for (int i = 0; i != CRC_POW_WORDS; ++i) {
    t.crc24b_pow32[i] = v;
    for (int s = 0; s != 32; ++s) {
      v <<= 1;
      if (v & top) {
        v ^= poly;
      }
    }
  }
  for (uint32_t b = 0; b != 256; ++b) {
    uint32_t r = b << 16;
    for (int k = 0; k != 8; ++k) {
      r <<= 1;
      if (r & top) {
        r ^= poly;
      }
    }
    t.crc24b_table[b] = r & (top - 1);
  }
  {
    auto mulx = [&](uint32_t a, unsigned e) { // a x^e mod g
      for (unsigned s = 0; s != e; ++s) {
        a <<= 1;
        if (a & top) {
          a ^= poly;
        }
      }
      return a;
    };
    for (unsigned m = 0; m != CRC_POW_WORDS; ++m) {
      for (unsigned n = 0; n != 6; ++n) {
        uint32_t e = mulx(t.crc24b_pow32[m], 4 * n); // x^(32 m + 4 n)
        // (v x^(4n)) x^(32m) for the 16 values of v, from the four single-bit products.
        uint32_t bit[4];
        for (unsigned k = 0; k != 4; ++k) {
          bit[k] = mulx(e, k);
        }
        for (uint32_t nib = 0; nib != 16; ++nib) {
          uint32_t acc = 0;
          for (unsigned k = 0; k != 4; ++k) {
            acc ^= ((nib >> k) & 1U) ? bit[k] : 0U;
          }
          t.crc24b_mul[m][n][nib] = acc;
        }
      }
    }
  }
  // Modulation tables: d = (1-2b0)[2^(h-1) - (1-2b2)[2^(h-2) - ...]] on the even bits, same on the odd bits for
  // the imaginary part (TS 38.211 Sections 5.1.3-5.1.6), h = Qm / 2.
  for (unsigned q = 0; q != 4; ++q) {
    const unsigned qm = 2 * (q + 1), h = q + 1;
    for (unsigned idx = 0; idx != (1U << qm); ++idx) {
      int re = 1 - 2 * (int)((idx >> 1) & 1U), im = 1 - 2 * (int)(idx & 1U);
      for (unsigned lvl = 1; lvl < h; ++lvl) {
        re = (1 - 2 * (int)((idx >> (2 * lvl + 1)) & 1U)) * ((1 << lvl) - re);
        im = (1 - 2 * (int)((idx >> (2 * lvl)) & 1U)) * ((1 << lvl) - im);
      }
      t.qam_lut[q][idx] = make_float2((float)re, (float)im);
    }
  }
  // x1(n + 1600), MSB-first words: x1(n+31) = x1(n+3) ^ x1(n), x1(0) = 1.
  x1_words.assign(GOLD_X1_WORDS, 0);
  uint32_t x1 = 1;
  for (int i = 0; i != 1600; ++i) {
    uint32_t f = ((x1 >> 3) ^ x1) & 1U;
    x1         = (x1 >> 1) | (f << 30);
  }
  for (size_t n = 0; n != (size_t)GOLD_X1_WORDS * 32; ++n) {
    if (x1 & 1U) {
      x1_words[n >> 5] |= 0x80000000U >> (n & 31);
    }
    uint32_t f = ((x1 >> 3) ^ x1) & 1U;
    x1         = (x1 >> 1) | (f << 30);
  }
}

} // namespace

struct nrphy_ofdm_plan {
  nrphy_ctx*          ctx = nullptr;
  nrphy_ofdm_config_t cfg;
  uint32_t            nof_ports = 0, nsymb = 14, slot_stride = 0, nsym_subframe = 0;
  const float2*       d_twiddle = nullptr; // the context's table of the DFT size
  float2*             d_phase = nullptr;
  float2*             d_phase_rx = nullptr; // demodulator: conjugate phase x scale (phase_compensation_lut, is_tx = false)
  uint32_t*           d_cp = nullptr;
  uint32_t*           d_off = nullptr;
  std::vector<uint32_t> cp, off;
  std::map<uint32_t, float2*> d_window_phase; // demodulator: per window offset, built on first use
  std::mutex          window_mutex;           // guards the map (the host-span entry points already hold ctx->host_mutex)
  std::vector<hipEvent_t> events; // 2 per recorded run
  uint32_t            timed_runs = 0, max_timed_runs = 0;
  uint32_t            timing_stride = 1, timing_counter = 0; // every timing_stride-th run is recorded
  uint4*              d_wire_partials = nullptr; // wire-format runs with measurements: one record per workgroup
  size_t              wire_partials_cap = 0;     // records
};

// ================================================================================================================
// Scalars
// ================================================================================================================
extern "C" const char* nrphy_version(void)
{
  return "mi355-nrphy 0.1 (gfx950)";
}

extern "C" int nrphy_trace_enabled(void)
{
  return trace_enabled() ? 1 : 0;
}

extern "C" const char* nrphy_strerror(int status)
{
  switch (status) {
    case NRPHY_OK:
      return "ok";
    case NRPHY_ERR_INVALID_PDU:
      return "invalid PDSCH PDU (pdsch_pdu_validator::is_valid is false)";
    case NRPHY_ERR_ARGUMENT:
      return "invalid argument";
    case NRPHY_ERR_DEVICE:
      return "HIP device error (no GPU or kernel launch failure); there is no CPU fallback";
    case NRPHY_ERR_CAPACITY:
      return "capacity exceeded";
    default:
      return "unknown status";
  }
}

namespace {

// cyclic_prefix::get_length + phy_time_unit::to_samples (R/include/srsran/ran/cyclic_prefix.h:93-104,
// phy_time_unit.h:100-111): units of kappa*Tc at 15 kHz -> samples at 15 kHz * 2^mu * dft_size.
unsigned cp_length(const nrphy_ofdm_config_t& c, unsigned symbol_index)
{
  const unsigned mu    = c.numerology;
  unsigned       units = 144U >> mu;
  if (c.cp) {
    units = 512U >> mu;
  } else if (symbol_index == 0 || symbol_index == 7U * (1U << mu)) {
    units += 16;
  }
  return (unsigned)(((uint64_t)units * c.dft_size * (1U << mu)) / 2048U);
}

} // namespace

extern "C" uint32_t nrphy_ofdm_symbol_size(const nrphy_ofdm_config_t* cfg, uint32_t symbol_index)
{
  return cp_length(*cfg, symbol_index) + cfg->dft_size;
}

extern "C" uint32_t nrphy_ofdm_slot_size(const nrphy_ofdm_config_t* cfg, uint32_t slot_index)
{
  const unsigned nsymb = cfg->cp ? 12 : 14;
  unsigned       n     = 0;
  for (unsigned l = 0; l != nsymb; ++l) {
    n += nrphy_ofdm_symbol_size(cfg, nsymb * slot_index + l);
  }
  return n;
}

// ================================================================================================================
// Context
// ================================================================================================================

Tunables read_tunables()
{
  Tunables t;
  auto     number = [](const char* name, int unset) {
    const char* e = std::getenv(name);
    return (e != nullptr && e[0] != 0) ? std::atoi(e) : unset;
  };
  t.cb_dispatch       = number("NRPHY_CB_DISPATCH", 0);
  t.crc_regions       = number("NRPHY_CRC_REGIONS", 0);
  t.scr_parts_big     = number("NRPHY_SCR_PARTS_BIG", 0);
  t.scr_words         = number("NRPHY_SCR_WORDS", -1);
  t.extras_nt         = (uint32_t)number("NRPHY_EXTRAS_NT", 1);
  t.prologue_order    = (uint32_t)number("NRPHY_PROLOGUE_ORDER", 0);
  t.decoder_pairs     = number("NRPHY_DECODER_PAIRS", -1);
  t.decoder_ldsmsg    = number("NRPHY_DECODER_LDSMSG", -1);
  t.decoder_slots_all = number("NRPHY_DECODER_SLOTS_ALL", 0) == 1;
#ifdef NRPHY_PROBES
  t.profile_stage = (uint32_t)number("NRPHY_PROFILE_STAGE", 0);
  t.ofdm_probe    = (uint32_t)number("NRPHY_OFDM_PROBE", 0);
#endif
  return t;
}

extern "C" int nrphy_create(nrphy_ctx_t** out, int device_id)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out      = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipSetDevice(device_id));
  nrphy_ctx* ctx = new (std::nothrow) nrphy_ctx;
  if (ctx == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  ctx->device = device_id;
  ctx->tune   = read_tunables();
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) {
      ctx->nof_cus = (uint32_t)prop.multiProcessorCount;
    }
  }
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return NRPHY_ERR_DEVICE;
  }
  std::vector<LiftedGraph> graphs(NOF_GRAPHS);
  for (unsigned bg = 1; bg <= 2; ++bg) {
    for (int i = 0; i != NOF_LIFTING_SIZES; ++i) {
      build_lifted_graph(bg, LIFTING_SIZES[i], graphs[(bg - 1) * NOF_LIFTING_SIZES + i]);
    }
  }
  GoldTables            gold;
  std::vector<uint32_t> x1;
  build_gold_tables(gold, x1);
  ctx->graphs = graphs;
  std::vector<TbCrcTables> tbcrc(1);
  build_tbcrc_tables(tbcrc[0]);
  if (upload(&ctx->d_tbcrc, tbcrc.data(), sizeof(TbCrcTables)) != hipSuccess ||
      upload(&ctx->d_graphs, graphs.data(), graphs.size() * sizeof(LiftedGraph)) != hipSuccess ||
      upload(&ctx->d_gold, &gold, sizeof(gold)) != hipSuccess ||
      upload(&ctx->d_x1, x1.data(), x1.size() * sizeof(uint32_t)) != hipSuccess) {
    nrphy_destroy(ctx);
    return NRPHY_ERR_DEVICE;
  }
  *out = ctx;
  return NRPHY_OK;
}

extern "C" int nrphy_destroy(nrphy_ctx_t* ctx)
{
  if (ctx == nullptr) {
    return NRPHY_OK;
  }
  (void)hipSetDevice(ctx->device);
  (void)hipFree(ctx->d_graphs);
  (void)hipFree(ctx->d_gold);
  (void)hipFree(ctx->d_tbcrc);
  for (void* b : ctx->scratch) {
    (void)hipFree(b);
  }
  for (DecoderGraph* g : ctx->d_dec_graph) {
    (void)hipFree(g);
  }
  for (uint32_t* a : ctx->d_dec_addr) {
    (void)hipFree(a);
  }
  for (auto& kv : ctx->d_dec_crc) {
    (void)hipFree(kv.second);
  }
  for (auto& kv : ctx->d_tb_crc_w) {
    (void)hipFree(kv.second);
  }
  (void)hipFree(ctx->d_x1);
  (void)hipFree(ctx->d_prach);
  for (auto& kv : ctx->d_twiddle) {
    (void)hipFree(kv.second);
  }
  if (ctx->stream) {
    (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
  return NRPHY_OK;
}

extern "C" int nrphy_synchronize(nrphy_ctx_t* ctx, void* stream)
{
  if (ctx == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipStreamSynchronize(stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

// exp(+j 2 pi k / N) computed in double precision and rounded once.
const float2* get_twiddle(nrphy_ctx* ctx, uint32_t size)
{
  if (!dft_size_supported(size)) {
    return nullptr;
  }
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  auto it = ctx->d_twiddle.find(size);
  if (it != ctx->d_twiddle.end()) {
    return it->second;
  }
  std::vector<float2> tw(size);
  for (uint32_t k = 0; k != size; ++k) {
    double ang = 2.0 * M_PI * (double)k / (double)size;
    tw[k]      = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  float2* d = nullptr;
  if (upload(&d, tw.data(), tw.size() * sizeof(float2)) != hipSuccess) {
    return nullptr;
  }
  ctx->d_twiddle[size] = d;
  return d;
}

namespace {

// The walk of ldpc_rate_dematcher_impl::allot_llrs (ldpc_rate_dematcher_impl.cpp:118-200) over the soft buffer, with
// the data taken out: which ranges it clears, fills, copies into and adds to, in its order.  Returns false when the
void build_dematch_ops(std::vector<DematchOp>& ops, unsigned block_length, unsigned buffer_length, unsigned k0,
                       unsigned nof_systematic, unsigned nof_filler, unsigned e, bool new_data)
{
  const unsigned nof_info = nof_systematic - nof_filler;
  bool           copying  = new_data;
  unsigned       pos = k0, taken = 0;
  ops.clear();
  auto emit = [&](uint32_t kind, unsigned begin, unsigned count, unsigned src) {
    if (count != 0) {
      ops.push_back({kind, begin, count, src});
    }
  };
  while (taken != e) {
    unsigned left = e - taken;
    if (pos < nof_info) {
      const unsigned n = std::min(nof_info - pos, left);
      if (copying) {
        emit(DEMATCH_ZERO, 0, pos, 0);
      }
      emit(copying ? DEMATCH_COPY : DEMATCH_COMBINE, pos, n, taken);
      pos += n;
      taken += n;
      left -= n;
    } else if (copying) {
      emit(DEMATCH_ZERO, 0, nof_info, 0);
    }
    if (copying) {
      emit(DEMATCH_FILL, nof_info, nof_filler, 0);
    }
    pos = std::max(pos, nof_systematic);
    const unsigned n = std::min(buffer_length - pos, left);
    emit(copying ? DEMATCH_COPY : DEMATCH_COMBINE, pos, n, taken);
    pos = (pos + n) % buffer_length;
    taken += n;
    if (taken != e) {
      copying = false;
    }
  }
  if (copying && pos != 0) {
    // the reference clears this many soft bits at the end of the full-length block, wherever the buffer ends
    emit(DEMATCH_ZERO, block_length - (buffer_length - pos), buffer_length - pos, 0);
  }
}

// n_outer groups (transport blocks) of n_cb codeblocks: codeblock (g, i) reads d_in + g * in_outer + i * in_stride and
// owns the soft buffer d_soft + g * soft_outer + i * soft_stride.
int rate_dematch_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb, uint32_t n_outer,
                       const int8_t* d_in, uint32_t in_stride_bytes, size_t in_outer, int8_t* d_soft,
                       uint32_t soft_stride_bytes, size_t soft_outer, int new_data, void* stream);

} // namespace

extern "C" int nrphy_ldpc_rate_dematch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb,
                                       const int8_t* d_in, uint32_t in_stride_bytes, int8_t* d_soft,
                                       uint32_t soft_stride_bytes, int new_data, void* stream)
{
  return rate_dematch_batch(ctx, cfg, n_cb, 1, d_in, in_stride_bytes, 0, d_soft, soft_stride_bytes, 0, new_data, stream);
}

namespace {

int rate_dematch_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb, uint32_t n_outer,
                       const int8_t* d_in, uint32_t in_stride_bytes, size_t in_outer, int8_t* d_soft,
                       uint32_t soft_stride_bytes, size_t soft_outer, int new_data, void* stream)
{
  if (ctx == nullptr || cfg == nullptr || d_in == nullptr || d_soft == nullptr ||
      (cfg->base_graph != 1 && cfg->base_graph != 2) || cfg->rv > 3 || lifting_position(cfg->lifting_size) < 0 ||
      (cfg->qm != 1 && cfg->qm != 2 && cfg->qm != 4 && cfg->qm != 6 && cfg->qm != 8) || cfg->rm_length == 0 ||
      cfg->rm_length > 35 * 8448 /* ldpc::MAX_CODEBLOCK_RM_SIZE */ || cfg->rm_length % cfg->qm != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  static const double shift_bg1[4] = {0, 17, 33, 56}, shift_bg2[4] = {0, 13, 25, 43};
  const unsigned      zc = cfg->lifting_size, n_short = (cfg->base_graph == 1) ? 66 : 50;
  const unsigned      block_length   = n_short * zc;
  const unsigned      buffer_length  = (cfg->nref > 0 && cfg->nref < block_length) ? cfg->nref : block_length;
  const unsigned      nof_systematic = (((cfg->base_graph == 1) ? 22 : 10) - 2) * zc;
  if (cfg->nof_filler_bits >= nof_systematic || buffer_length <= nof_systematic || in_stride_bytes < cfg->rm_length ||
      soft_stride_bytes < block_length) {
    return NRPHY_ERR_ARGUMENT;
  }
  // ldpc_rate_dematcher_impl.cpp:94-95: k0 of TS 38.212 Table 5.4.2.1-2 in double precision
  const double   frac = (((cfg->base_graph == 1) ? shift_bg1 : shift_bg2)[cfg->rv] * buffer_length) / block_length;
  const unsigned k0   = (unsigned)((uint16_t)std::floor(frac)) * zc;
  DematchLaunch          p;
  std::vector<DematchOp> ops;
  build_dematch_ops(ops, block_length, buffer_length, k0, nof_systematic, cfg->nof_filler_bits, cfg->rm_length,
                    new_data != 0);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t   s = stream ? (hipStream_t)stream : ctx->stream;
  StreamStaging staging(s);
  p.n_ops   = (uint32_t)ops.size();
  p.ops_ext = nullptr;
  if (ops.size() <= MAX_DEMATCH_OPS) {
    std::copy(ops.begin(), ops.end(), p.ops);
  } else {
    // Heavy repetition (rm_length of dozens of buffer lengths): the list goes through device memory of this call's
    // own, allocated, filled and released in stream order.
    DematchOp* d_ops = (DematchOp*)staging.alloc(ops.size() * sizeof(DematchOp));
    if (d_ops == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
    HIP_TRY(hipMemcpyAsync(d_ops, ops.data(), ops.size() * sizeof(DematchOp), hipMemcpyHostToDevice, s));
    p.ops_ext = d_ops;
  }
  {
    // Do the copying / clearing / filling operations cover the whole block?  Then no soft bit keeps its old value and the
    // kernel skips reading the buffer (always so for a first transmission that does not wrap; never with combining).
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    bool combines = false;
    for (const DematchOp& op : ops) {
      combines = combines || op.kind == DEMATCH_COMBINE;
      ranges.emplace_back(op.begin, op.begin + op.count);
    }
    std::sort(ranges.begin(), ranges.end());
    uint32_t reach = 0;
    for (const auto& r : ranges) {
      if (r.first > reach) {
        break;
      }
      reach = std::max(reach, r.second);
    }
    p.skip_load = (!combines && reach >= block_length) ? 1U : 0U;
    // Pairwise disjoint destination ranges (sorted by begin: each starts where the previous one has ended or later)?
    p.disjoint = 1U;
    for (size_t i = 1; i < ranges.size(); ++i) {
      if (ranges[i].first < ranges[i - 1].second) {
        p.disjoint = 0U;
      }
    }
  }
  p.in           = d_in;
  p.out          = d_soft;
  p.in_stride    = in_stride_bytes;
  p.out_stride   = soft_stride_bytes;
  p.block_length = block_length;
  p.qm           = cfg->qm;
  p.cols         = cfg->rm_length / cfg->qm;
  p.in_stride_outer  = (uint32_t)in_outer;
  p.out_stride_outer = (uint32_t)soft_outer;
  if (in_outer > 0xFFFFFFFFULL || soft_outer > 0xFFFFFFFFULL) {
    return NRPHY_ERR_CAPACITY;
  }
  HIP_TRY(launch_ldpc_dematch(p, n_cb, s, n_outer));
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ldpc_rate_dematch_host(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg,
                                            const int8_t* in, int8_t* soft_buffer, int new_data)
{
  // Everything that sizes a copy below is checked here, before the validating device-pointer call runs.
  if (ctx == nullptr || cfg == nullptr || in == nullptr || soft_buffer == nullptr ||
      (cfg->base_graph != 1 && cfg->base_graph != 2) || lifting_position(cfg->lifting_size) < 0 || cfg->rm_length == 0 ||
      cfg->rm_length > 35 * 8448) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned block_length = ((cfg->base_graph == 1) ? 66U : 50U) * cfg->lifting_size;
  HostCall       call(ctx);
  uint8_t*       d[2]; // in, soft buffer
  if (!call.carve(SCRATCH_RX, {(size_t)cfg->rm_length + 16, (size_t)block_length + 16}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  int8_t *d_in = (int8_t*)d[0], *d_soft = (int8_t*)d[1];
  HIP_TRY(hipMemcpy(d_in, in, cfg->rm_length, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_soft, soft_buffer, block_length, hipMemcpyHostToDevice));
  const int rc = nrphy_ldpc_rate_dematch(ctx, cfg, 1, d_in, cfg->rm_length, d_soft, block_length, new_data, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(soft_buffer, d_soft, block_length, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

namespace {

// Label bit k of a Gray-mapped PAM level (TS 38.211 Section 5.1): bit 0 is the sign; bit k >= 1 is set in the outer half of
// the magnitude's current range, which then folds around its middle.
unsigned pam_label_bit(int level, unsigned k, unsigned m)
{
  if (k == 0) {
    return level < 0;
  }
  int t = std::abs(level), r = 1 << m;
  for (unsigned j = 1;; ++j) {
    const unsigned bit = t > r / 2;
    if (j == k) {
      return bit;
    }
    t = std::abs(t - r / 2);
    r /= 2;
  }
}

// Max-log LLR of bit pair k as a piecewise-linear function on n intervals of width_units / sqrt(norm): in the interval whose
// nearest points with the bit 0 / 1 are a0 / a1, LLR(v) = 2 (a0 - a1) v + (a1^2 - a0^2).  The values are those of the
// reference's tables (demodulation_mapper_qam64.cpp:49-92, demodulation_mapper_qam256.cpp:47-160), derived, not copied.
void demod_interval_table(DemodLaunch& p, unsigned pair, unsigned m, float a, unsigned norm, unsigned width_units, unsigned n)
{
  const int M            = 1 << m;
  p.nof_intervals[pair]  = n;
  p.width[pair]          = (float)width_units * a;
  p.rcp_width[pair]      = 1.0F / p.width[pair];
  for (unsigned j = 0; j != n; ++j) {
    const double centre = ((double)j - (double)n / 2 + 0.5) * (double)width_units;
    int          a0 = 0, a1 = 0;
    double       d0 = 1e30, d1 = 1e30;
    for (int q = 0; q != M; ++q) {
      const int    level = 2 * q - (M - 1);
      const double d     = std::fabs(centre - level);
      if (pam_label_bit(level, pair, m)) {
        if (d < d1) {
          d1 = d, a1 = level;
        }
      } else if (d < d0) {
        d0 = d, a0 = level;
      }
    }
    p.slope[pair][j]     = (float)(2 * (a0 - a1)) * a;
    p.intercept[pair][j] = (float)(a1 * a1 - a0 * a0) / (float)norm;
  }
}

bool demod_launch_params(uint32_t modulation, uint32_t span_len, DemodLaunch& p)
{
  std::memset(&p, 0, sizeof(p));
  p.modulation = modulation;
  p.span_len   = span_len;
  uint32_t batch = 0;
  switch (modulation) {
    case NRPHY_MOD_PI2_BPSK:
    case NRPHY_MOD_BPSK:
      p.range = 24.0F;
      break;
    case NRPHY_MOD_QPSK:
      p.range = 24.0F;
      batch   = 16;
      break;
    case NRPHY_MOD_QAM16:
      p.range           = 20.0F;
      batch             = 8;
      p.qam16_gain      = 4.0F * (1.0F / std::sqrt(10.0F));
      p.qam16_threshold = 2 * (1.0F / std::sqrt(10.0F));
      break;
    case NRPHY_MOD_QAM64: {
      p.range       = 20.0F;
      batch         = 16;
      const float a = 1.0F / std::sqrt(42.0F);
      demod_interval_table(p, 0, 3, a, 42, 2, 8);
      demod_interval_table(p, 1, 3, a, 42, 2, 8);
      demod_interval_table(p, 2, 3, a, 42, 4, 4);
      break;
    }
    case NRPHY_MOD_QAM256: {
      p.range       = 20.0F;
      batch         = 4;
      const float a = 1.0F / std::sqrt(170.0F);
      demod_interval_table(p, 0, 4, a, 170, 2, 16);
      demod_interval_table(p, 1, 4, a, 170, 2, 16);
      demod_interval_table(p, 2, 4, a, 170, 2, 16);
      demod_interval_table(p, 3, 4, a, 170, 4, 8);
      break;
    }
    default:
      return false;
  }
  p.scale      = 120.0F / p.range;
  p.nof_vector = batch ? span_len / batch * batch : 0;
  return true;
}

} // namespace

bool nrphy::demod_params(uint32_t modulation, uint32_t span_len, DemodLaunch& p)
{
  return demod_launch_params(modulation, span_len, p);
}

extern "C" int nrphy_demodulate_soft(nrphy_ctx_t* ctx, uint32_t modulation, uint32_t nof_spans, uint32_t span_len,
                                     const float* d_symbols, const float* d_noise_vars, int8_t* d_llr, void* stream)
{
  DemodLaunch p;
  if (ctx == nullptr || !demod_launch_params(modulation, span_len, p) || nof_spans > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (nof_spans == 0 || span_len == 0) {
    return NRPHY_OK;
  }
  if (d_symbols == nullptr || d_noise_vars == nullptr || d_llr == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_demodulate_soft(p, nof_spans, d_symbols, d_noise_vars, d_llr, stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_demodulate_soft_host(nrphy_ctx_t* ctx, uint32_t modulation, uint32_t nof_symbols, const float* symbols,
                                          const float* noise_vars, int8_t* llr)
{
  DemodLaunch p;
  if (ctx == nullptr || !demod_launch_params(modulation, nof_symbols, p)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (nof_symbols == 0) {
    return NRPHY_OK;
  }
  if (symbols == nullptr || noise_vars == nullptr || llr == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t              qm = modulation == NRPHY_MOD_PI2_BPSK ? 1U : modulation;
  HostCall call(ctx);
  uint8_t* d[3]; // symbols, noise variances, soft bits
  if (!call.carve(SCRATCH_RX, {(size_t)nof_symbols * 8, (size_t)nof_symbols * 4, (size_t)nof_symbols * qm + 16}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  float * d_sym = (float*)d[0], *d_nv = (float*)d[1];
  int8_t* d_out = (int8_t*)d[2];
  HIP_TRY(hipMemcpyAsync(d_sym, symbols, (size_t)nof_symbols * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(d_nv, noise_vars, (size_t)nof_symbols * 4, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_demodulate_soft(ctx, modulation, 1, nof_symbols, d_sym, d_nv, d_out, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(llr, d_out, (size_t)nof_symbols * qm, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_llr_descramble(nrphy_ctx_t* ctx, uint32_t n_cw, const uint32_t* d_c_init, uint32_t length,
                                    const int8_t* d_in, size_t in_stride, int8_t* d_out, size_t out_stride, void* stream)
{
  if (ctx == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (n_cw == 0 || length == 0) {
    return NRPHY_OK;
  }
  // The x1 table holds the first 2^21 sequence bits (the longest PUSCH / PDSCH codeword is 1.47 Mbit).
  if (d_c_init == nullptr || d_in == nullptr || d_out == nullptr || length > (uint32_t)GOLD_X1_WORDS * 32U ||
      (n_cw > 1 && (in_stride < length || out_stride < length)) || n_cw > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_llr_descramble(ctx->d_gold, ctx->d_x1, d_c_init, n_cw, length, d_in, in_stride, d_out, out_stride,
                                stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_llr_descramble_host(nrphy_ctx_t* ctx, uint32_t c_init, uint32_t length, const int8_t* in, int8_t* out)
{
  if (ctx == nullptr || (length != 0 && (in == nullptr || out == nullptr))) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (length == 0) {
    return NRPHY_OK;
  }
  HostCall call(ctx);
  uint8_t* d[2]; // soft bits, c_init
  if (!call.carve(SCRATCH_RX, {(size_t)length + 16, 16}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  int8_t*   d_buf = (int8_t*)d[0];
  uint32_t* d_ci  = (uint32_t*)d[1];
  HIP_TRY(hipMemcpy(d_buf, in, length, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ci, &c_init, sizeof(c_init), hipMemcpyHostToDevice));
  const int rc = nrphy_llr_descramble(ctx, 1, d_ci, length, d_buf, length, d_buf, length, ctx->stream); // in place, as the caller does
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(out, d_buf, length, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

namespace {

// Decoder graph of (base graph, lifting size): all edges of TS 38.212 Tables 5.3.2-2/-3, row by row.
const DecoderGraph* get_decoder_graph(nrphy_ctx* ctx, unsigned bg, unsigned zc)
{
  const int pos = lifting_position(zc);
  if (pos < 0) {
    return nullptr;
  }
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
  return pos < 0 ? nullptr : ctx->d_dec_addr[(bg - 1) * NOF_LIFTING_SIZES + (unsigned)pos];
}

// Early-stop tables: word w of the n-bit message (32 bits, the last one n mod 32) is followed by n - 32 w - bits(w)
// bits; the message is a multiple of the generator g iff the sum of word(w) * x^(that) vanishes mod g.  Per word eight
// nibble tables, tab[w][k][v] = (v x^(4 k)) * x^(bits after word w) mod g: the product is eight independent look-ups
// instead of a 32-step shift-and-add per word and iteration (which was about 15 % of an early-stop iteration).
const uint32_t* get_decoder_crc_weights(nrphy_ctx* ctx, uint32_t poly, uint32_t order, uint32_t n_msg)
{
  const uint64_t key = ((uint64_t)poly << 32) | n_msg;
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

} // namespace

namespace {
// skip / ok_flags: per-codeblock HARQ state of a transport-block decoder; crc_at_end: no early stop.
// expected_extent: how many of the nof_llr soft bits the caller expects to be in use (the rest zero), 0 = all of them; it
// only sizes the launch's LDS (messages per edge in LDS when the layers that extent needs are few), never the result.
int ldpc_decode_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_decoder_cfg_t* cfg, uint32_t n_cb, const int8_t* d_llr,
                      uint32_t llr_stride_bytes, uint8_t* d_out, uint32_t out_stride_bytes, uint32_t* d_iterations,
                      const uint8_t* d_skip, uint8_t* d_ok_flags, bool crc_at_end, void* d_scratch, void* stream,
                      uint32_t expected_extent = 0);

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
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
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

namespace {

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
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
    p.graph     = get_decoder_graph(ctx, cfg->base_graph, zc);
    p.pair_addr = get_decoder_pair_addresses(ctx, cfg->base_graph, zc);
  }
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
    std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
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

} // namespace

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

// ================================================================================================================
// PUSCH decoder, transport-block level
// ================================================================================================================
namespace {

struct PuschLayout {
  nrphy_pdsch_derived_t d;
  uint32_t              msg_stride; // bytes per decoded message
  uint64_t              off_ok, off_skip, off_iter, off_msg, state_bytes;
};

bool pusch_layout(const nrphy_pusch_decoder_cfg_t& cfg, uint32_t n_tb, PuschLayout& l)
{
  if ((cfg.base_graph != 1 && cfg.base_graph != 2) || (cfg.qm != 1 && cfg.qm != 2 && cfg.qm != 4 && cfg.qm != 6 && cfg.qm != 8) ||
      cfg.rv > 3 || cfg.nof_layers == 0 || cfg.nof_layers > NRPHY_MAX_LAYERS || cfg.tb_size_bytes == 0 ||
      cfg.tb_size_bytes > NRPHY_MAX_TB_BYTES || cfg.nof_ch_symbols == 0 || cfg.nof_ch_symbols % cfg.nof_layers != 0 || cfg.max_iterations == 0) {
    return false;
  }
  // Segmentation is the transmitter's (ldpc_segmenter_rx_impl mirrors ldpc_segmenter_tx): reuse its derivation.
  nrphy_pdsch_pdu_t pdu;
  std::memset(&pdu, 0, sizeof(pdu));
  pdu.ldpc_base_graph = cfg.base_graph;
  pdu.tb_size_bytes   = cfg.tb_size_bytes;
  pdu.rv              = cfg.rv;
  pdu.nof_layers      = cfg.nof_layers;
  pdu.qm              = cfg.qm;
  const uint32_t nref = cfg.nref;
  derive(pdu, cfg.nof_ch_symbols / cfg.nof_layers, l.d, &nref);
  if (l.d.lifting_size == 0 || l.d.nof_codeblocks == 0 || l.d.nof_codeblocks > NRPHY_MAX_CODEBLOCKS ||
      l.d.rm_length_short == 0) {
    return false;
  }
  const uint64_t n_cb = (uint64_t)n_tb * l.d.nof_codeblocks;
  l.msg_stride        = ((l.d.segment_length + 7) / 8 + 8 + 15) & ~15U;
  l.off_ok            = 0;
  l.off_skip          = (n_cb + 63) & ~(uint64_t)63;
  l.off_iter          = 2 * l.off_skip;
  l.off_msg           = (l.off_iter + 4 * n_cb + 63) & ~(uint64_t)63;
  l.state_bytes       = l.off_msg + n_cb * l.msg_stride;
  return true;
}

} // namespace

namespace {
// Weights of the assembly kernel's per-thread transport-block CRC pieces (pusch_decoder.hip): fixed by the block size.
const uint32_t* get_pusch_tb_crc_weights(nrphy_ctx* ctx, uint32_t tb_size_bytes)
{
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  auto                                  it = ctx->d_tb_crc_w.find(tb_size_bytes);
  if (it == ctx->d_tb_crc_w.end()) {
    const uint32_t        piece = divide_ceil(tb_size_bytes, PUSCH_ASSEMBLE_THREADS);
    std::vector<uint32_t> w(PUSCH_ASSEMBLE_THREADS);
    for (uint32_t t = 0; t != PUSCH_ASSEMBLE_THREADS; ++t) {
      const uint32_t end = std::min<uint32_t>(std::min<uint32_t>(t * piece, tb_size_bytes) + piece, tb_size_bytes);
      w[t]               = CRC24A_FIELD.xpow(8 * (int64_t)(tb_size_bytes - end));
    }
    uint32_t* d_w = nullptr;
    if (upload(&d_w, w.data(), w.size() * sizeof(uint32_t)) != hipSuccess) {
      return nullptr;
    }
    it = ctx->d_tb_crc_w.emplace(tb_size_bytes, d_w).first;
  }
  return it->second;
}

nrphy_ldpc_decoder_cfg_t pusch_ldpc_cfg(const nrphy_pusch_decoder_cfg_t& cfg, const nrphy_pdsch_derived_t& d)
{
  // Decoding of the codeblocks whose CRC has not passed yet (pusch_codeblock_decoder.cpp:36-71): CRC24B per codeblock,
  // the transport block's own CRC when it is a single codeblock.
  nrphy_ldpc_decoder_cfg_t dec;
  dec.base_graph      = cfg.base_graph;
  dec.lifting_size    = d.lifting_size;
  dec.nof_filler_bits = d.nof_filler_bits;
  dec.crc_poly        = (d.nof_codeblocks > 1) ? 0x24B : (d.nof_tb_crc_bits == 16 ? 16 : 0x24A);
  dec.nof_llr         = d.full_length;
  dec.max_iterations  = cfg.max_iterations;
  dec.scaling_factor  = 0.8F; // ldpc_decoder::configuration::algorithm_details default, which pusch_codeblock_decoder keeps
  return dec;
}
} // namespace

extern "C" int nrphy_pusch_decoder_prepare(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg)
{
  PuschLayout l;
  if (ctx == nullptr || cfg == nullptr || !pusch_layout(*cfg, 1, l)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, l.d);
  const int                      rc  = nrphy_ldpc_decoder_prepare(ctx, &dec);
  if (rc != NRPHY_OK) {
    return rc;
  }
  if (l.d.nof_codeblocks > 1 && get_pusch_tb_crc_weights(ctx, cfg->tb_size_bytes) == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_decoder_sizes(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb,
                                         uint64_t* soft_bytes_per_tb, uint64_t* state_bytes, uint64_t* scratch_bytes,
                                         uint32_t* nof_codeblocks)
{
  PuschLayout l;
  if (ctx == nullptr || cfg == nullptr || !pusch_layout(*cfg, n_tb, l)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (scratch_bytes) {
    const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, l.d);
    if (nrphy_ldpc_decoder_scratch_bytes(ctx, &dec, std::max<uint32_t>(1, n_tb * l.d.nof_codeblocks), scratch_bytes) != NRPHY_OK) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  if (soft_bytes_per_tb) {
    *soft_bytes_per_tb = (uint64_t)l.d.nof_codeblocks * l.d.full_length;
  }
  if (state_bytes) {
    *state_bytes = l.state_bytes;
  }
  if (nof_codeblocks) {
    *nof_codeblocks = l.d.nof_codeblocks;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_decode_batch(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb,
                                        const int8_t* d_llr, uint64_t llr_stride_bytes, int8_t* d_soft, uint8_t* d_state,
                                        void* d_scratch, uint8_t* d_tb, uint32_t tb_stride_bytes, uint32_t* d_result, void* stream)
{
  const TraceRange trace("process_pusch");
  PuschLayout l;
  if (ctx == nullptr || cfg == nullptr || d_llr == nullptr || d_soft == nullptr || d_state == nullptr || d_tb == nullptr ||
      d_scratch == nullptr ||
      d_result == nullptr || !pusch_layout(*cfg, n_tb, l) || tb_stride_bytes < cfg->tb_size_bytes ||
      llr_stride_bytes < (uint64_t)cfg->nof_ch_symbols * cfg->qm) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (n_tb == 0) {
    return NRPHY_OK;
  }
  const nrphy_pdsch_derived_t& d = l.d;
  const uint32_t               C = d.nof_codeblocks, N = d.full_length;
  const uint64_t               n_cb = (uint64_t)n_tb * C;
  hipStream_t                  s    = stream ? (hipStream_t)stream : ctx->stream;
  uint8_t *                    ok = d_state + l.off_ok, *skip = d_state + l.off_skip, *msg = d_state + l.off_msg;
  uint32_t*                    iter = (uint32_t*)(d_state + l.off_iter);
  HIP_TRY(hipSetDevice(ctx->device));
  if (cfg->new_data) { // a fresh soft buffer has no codeblock CRC flags
    HIP_TRY(hipMemsetAsync(ok, 0, n_cb, s));
  }
  HIP_TRY(hipMemcpyAsync(skip, ok, n_cb, hipMemcpyDeviceToDevice, s));
  // Rate dematching of every codeblock, also of those decoded earlier (pusch_decoder_impl.cpp:340-350): the short
  // segments, then the long ones.
  nrphy_ldpc_rate_dematcher_cfg_t dm;
  dm.base_graph      = cfg->base_graph;
  dm.lifting_size    = d.lifting_size;
  dm.rv              = cfg->rv;
  dm.qm              = cfg->qm;
  dm.nref            = d.n_ref;
  dm.nof_filler_bits = d.nof_filler_bits;
  const uint32_t n_short = d.nof_short_segments;
  int            rc      = NRPHY_OK;
  if (n_short != 0) {
    dm.rm_length = d.rm_length_short;
    rc = rate_dematch_batch(ctx, &dm, n_short, n_tb, d_llr, d.rm_length_short, llr_stride_bytes, d_soft, N, (size_t)C * N,
                            cfg->new_data, s);
  }
  if (rc == NRPHY_OK && n_short != C) {
    dm.rm_length = d.rm_length_long;
    rc = rate_dematch_batch(ctx, &dm, C - n_short, n_tb, d_llr + (size_t)n_short * d.rm_length_short, d.rm_length_long,
                            llr_stride_bytes, d_soft + (size_t)n_short * N, N, (size_t)C * N, cfg->new_data, s);
  }
  if (rc != NRPHY_OK) {
    return rc;
  }
  const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, d);
  // How far into the soft buffers a first transmission reaches (filler bits included): what the decoder can expect to be in
  // use when the buffers held nothing else -- a hint for the launch's LDS size only (see ldpc_decode_batch).
  uint32_t expected_extent = 0;
  if (cfg->new_data) {
    const unsigned bg_k = (cfg->base_graph == 1) ? 22 : 10, zc = d.lifting_size;
    const unsigned buffer_length = (d.n_ref > 0 && d.n_ref < N) ? d.n_ref : N;
    static const double shift_bg1[4] = {0, 17, 33, 56}, shift_bg2[4] = {0, 13, 25, 43};
    const double   frac = (((cfg->base_graph == 1) ? shift_bg1 : shift_bg2)[cfg->rv] * buffer_length) / N;
    const unsigned k0   = (unsigned)((uint16_t)std::floor(frac)) * zc;
    std::vector<DematchOp> ops;
    for (uint32_t e : {d.rm_length_short, d.rm_length_long}) {
      if (e == 0) {
        continue;
      }
      build_dematch_ops(ops, N, buffer_length, k0, (bg_k - 2) * zc, d.nof_filler_bits, e, true);
      for (const DematchOp& op : ops) {
        if (op.kind != DEMATCH_ZERO) {
          expected_extent = std::max<uint32_t>(expected_extent, op.begin + op.count);
        }
      }
    }
  }
  rc = ldpc_decode_batch(ctx, &dec, (uint32_t)n_cb, d_soft, N, msg, l.msg_stride, iter, skip, ok, cfg->use_early_stop == 0,
                         d_scratch, s, expected_extent);
  if (rc != NRPHY_OK) {
    return rc;
  }
  PuschAssembleLaunch a;
  a.crc_weight = nullptr;
  if (C > 1) {
    a.crc_weight = get_pusch_tb_crc_weights(ctx, cfg->tb_size_bytes); // uploaded by nrphy_pusch_decoder_prepare() or here
    if (a.crc_weight == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  a.cb_msg         = msg;
  a.cb_ok          = ok;
  a.cb_iter        = iter;
  a.skipped        = skip;
  a.tb             = d_tb;
  a.result         = d_result;
  a.C              = C;
  a.msg_stride     = l.msg_stride;
  a.tb_stride      = tb_stride_bytes;
  a.tb_bytes       = cfg->tb_size_bytes;
  a.cb_info_bits   = d.cb_info_bits;
  a.max_iterations = cfg->max_iterations;
  // The transport-block check by 16 KiB regions (tbcrc_regions_workgroup, the transmit side's TB-CRC role): the context's
  // tables and the factor that turns the remainder of the zero-extended block into the block's CRC24A.
  a.tbcrc          = ctx->d_tbcrc;
  a.crc_factor     = CRC24A_FIELD.xpow((int64_t)CRC24A_FIELD.order +
                                   8 * ((int64_t)cfg->tb_size_bytes -
                                        (int64_t)divide_ceil(cfg->tb_size_bytes, TB_CRC_REGION_BYTES) * TB_CRC_REGION_BYTES));
  HIP_TRY(launch_pusch_assemble(a, n_tb, s));
  return NRPHY_OK;
}

// ================================================================================================================
// NZP-CSI-RS
// ================================================================================================================
extern "C" int nrphy_csi_rs_validate(const nrphy_csi_rs_cfg_t* c)
{
  static const unsigned row_ports[6] = {0, 1, 1, 2, 4, 4};
  if (c == nullptr || c->row < 1 || c->row > 5 || c->nof_k_ref != 1 || c->cp > 1 || c->nof_rb == 0 ||
      c->nof_ports != row_ports[c->row] || c->precoding == nullptr || c->nof_prg != 1 || c->prg_size_rb == 0 || c->prg_size_rb > NRPHY_MAX_RB ||
      c->start_rb + c->nof_rb > NRPHY_MAX_RB) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The assertions of mapping_row_1 .. mapping_row_5 (csi_rs_pattern.cpp:34-158); densities as csi_rs_freq_density_type.
  const unsigned nsymb = c->cp ? 12 : 14, k0 = c->k_ref[0];
  const bool     three = c->density == 3, one = c->density == 2, valid_density = c->density <= 3;
  bool           ok    = false;
  switch (c->row) {
    case 1:
      ok = k0 <= 3 && three && c->cdm == 0 && c->symbol_l0 < nsymb;
      break;
    case 2:
      ok = k0 < 12 && valid_density && !three && c->cdm == 0 && c->symbol_l0 < nsymb;
      break;
    case 3:
      ok = k0 < 11 && valid_density && !three && c->cdm == 1 && c->symbol_l0 < nsymb;
      break;
    case 4:
      ok = k0 < 9 && one && c->cdm == 1 && c->symbol_l0 < nsymb;
      break;
    default:
      ok = k0 < 11 && one && c->cdm == 1 && c->symbol_l0 + 1 < nsymb;
      break;
  }
  return ok ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

extern "C" int nrphy_csi_rs_map(nrphy_ctx_t* ctx, uint32_t n, const nrphy_csi_rs_cfg_t* cfgs, const uint32_t* grid_index,
                                void* d_grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* stream)
{
  const TraceRange trace("process_nzp_csi_rs");
  if (ctx == nullptr || (n != 0 && (cfgs == nullptr || d_grid == nullptr))) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<CsiRsWork> work;
  std::vector<float>     weights;
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_csi_rs_cfg_t& c = cfgs[i];
    if (nrphy_csi_rs_validate(&c) != NRPHY_OK || c.nof_ports > grid_nof_ports || 12 * (c.start_rb + c.nof_rb) > grid_nof_subc) {
      return NRPHY_ERR_ARGUMENT;
    }
    const unsigned group_size = c.cdm ? 2 : 1, nof_groups = c.nof_ports / group_size;
    const bool     half       = c.density <= 1, even = c.density == 0;
    // PRB range and stride (build_re_patterns, csi_rs_pattern.cpp:374-392)
    unsigned rb_begin = c.start_rb, rb_stride = half ? 2 : 1;
    if (half && (((c.start_rb % 2) != 0) == even)) {
      ++rb_begin;
    }
    // sequence elements below the first occupied PRB and per symbol (nzp_csi_rs_generator_impl.cpp:66-159)
    unsigned first_prb = c.start_rb;
    if (half) {
      first_prb = even ? c.start_rb + c.start_rb % 2 : c.start_rb + (1 - c.start_rb % 2);
    }
    unsigned advance = 0;
    if (c.density == 3) {
      advance = 3 * first_prb;
    } else if (c.density == 2) {
      advance = (c.row == 2) ? first_prb : 2 * first_prb;
    } else {
      advance = (c.row == 2) ? first_prb / 2 : first_prb;
    }
    unsigned seq_len = c.nof_rb;
    if (half) {
      seq_len /= 2;
      if (c.nof_rb % 2 != 0 && (((c.start_rb % 2) != 0) == !even)) {
        ++seq_len;
      }
    } else if (c.density == 3) {
      seq_len *= 3;
    }
    seq_len *= c.cdm ? 2 : 1;
    const unsigned nsymb = c.cp ? 12 : 14;
    for (unsigned g = 0; g != nof_groups; ++g) {
      CsiRsWork w;
      unsigned  k_bar = c.k_ref[0], l_bar = c.symbol_l0;
      if (c.row == 4) {
        k_bar += 2 * g;
      } else if (c.row == 5) {
        l_bar += g;
      }
      w.re_mask    = (c.row == 1) ? ((1U << k_bar) | (1U << (k_bar + 4)) | (1U << (k_bar + 8))) : ((c.cdm ? 3U : 1U) << k_bar);
      w.n_re_prb   = (uint32_t)__builtin_popcount(w.re_mask);
      w.grid_index = grid_index ? grid_index[i] : 0;
      w.symbol     = l_bar;
      w.c_init     = (uint32_t)((1024ULL * (nsymb * c.slot_index + l_bar + 1) * (2 * c.scrambling_id + 1) + c.scrambling_id) & 0x7FFFFFFFULL);
      w.advance    = advance;
      w.seq_len    = seq_len;
      w.rb_begin   = rb_begin;
      w.rb_stride  = rb_stride;
      w.nof_ports  = c.nof_ports;
      w.first_layer = g * group_size;
      w.group_size  = group_size;
      w.weights_offset = (uint32_t)weights.size();
      w.amplitude   = (float)(M_SQRT1_2 * (double)c.amplitude);
      if (2 * (advance + seq_len) + 32 > 32 * CSI_RS_MAX_SEQ_WORDS) {
        return NRPHY_ERR_CAPACITY;
      }
      work.push_back(w);
    }
    weights.insert(weights.end(), c.precoding, c.precoding + 2 * (size_t)c.nof_ports * c.nof_ports);
  }
  if (work.empty()) {
    return NRPHY_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // Work list and weights go through a buffer of this call's own (stream-ordered allocation).
  const size_t  work_bytes = work.size() * sizeof(CsiRsWork), off_w = (work_bytes + 63) & ~(size_t)63;
  StreamStaging staging(s);
  uint8_t*      base = (uint8_t*)staging.alloc(off_w + weights.size() * sizeof(float));
  if (base == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  // pageable host memory: hipMemcpyAsync stages it before returning, the vectors may go out of scope
  HIP_TRY(hipMemcpyAsync(base, work.data(), work_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(base + off_w, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice, s));
  CsiRsLaunch p;
  p.work           = (const CsiRsWork*)base;
  p.weights        = (const float*)(base + off_w);
  p.gold           = ctx->d_gold;
  p.x1_words       = ctx->d_x1;
  p.grid           = (uint32_t*)d_grid;
  p.grid_nof_ports = grid_nof_ports;
  p.grid_nof_subc  = grid_nof_subc;
  HIP_TRY(launch_csi_rs(p, (uint32_t)work.size(), s));
  return NRPHY_OK;
}

extern "C" int nrphy_csi_rs_map_host(nrphy_ctx_t* ctx, const nrphy_csi_rs_cfg_t* cfg, void* grid, uint32_t nof_ports,
                                     uint32_t nof_subc)
{
  if (ctx == nullptr || cfg == nullptr || grid == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall     call(ctx);
  const size_t bytes  = (size_t)nof_ports * NRPHY_NSYMB * nof_subc * 4;
  void*        d_grid = call.mem(SCRATCH_GRID, bytes);
  if (d_grid == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(d_grid, grid, bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_csi_rs_map(ctx, 1, cfg, nullptr, d_grid, nof_ports, nof_subc, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(grid, d_grid, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_grid_put(nrphy_ctx_t* ctx, void* d_grid, uint32_t nof_ports, uint32_t nof_subc, uint32_t n,
                              const nrphy_grid_re_t* entries, void* stream)
{
  if (ctx == nullptr || d_grid == nullptr || (n != 0 && entries == nullptr) || nof_ports > NRPHY_MAX_PORTS ||
      nof_subc > NRPHY_MAX_RB * 12) { // (also keeps the 32-bit element index below from wrapping)
    return NRPHY_ERR_ARGUMENT;
  }
  if (n == 0) {
    return NRPHY_OK;
  }
  std::vector<uint32_t> packed(2 * (size_t)n);
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_grid_re_t& e = entries[i];
    if (e.port >= nof_ports || e.symbol >= NRPHY_NSYMB || e.subc >= nof_subc) {
      return NRPHY_ERR_ARGUMENT;
    }
    packed[i]     = ((uint32_t)e.port * NRPHY_NSYMB + e.symbol) * nof_subc + e.subc;
    packed[n + i] = e.value;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s    = stream ? (hipStream_t)stream : ctx->stream;
  StreamStaging staging(s);
  uint32_t*     base = (uint32_t*)staging.alloc(packed.size() * sizeof(uint32_t));
  if (base == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpyAsync(base, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_grid_put(base, base + n, n, (uint32_t*)d_grid, s));
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_encode(nrphy_ctx_t* ctx, uint32_t base_graph, uint32_t lifting_size, uint32_t n_cb,
                                 const uint8_t* d_msg, uint32_t msg_stride_bytes, uint32_t out_bits, uint8_t* d_out,
                                 uint32_t out_stride_bytes, void* stream)
{
  if (ctx == nullptr || (base_graph != 1 && base_graph != 2) || d_msg == nullptr || d_out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const int pos = lifting_position(lifting_size);
  const unsigned kb = (base_graph == 1) ? 22 : 10, nfull = (base_graph == 1) ? 68 : 52;
  if (pos < 0 || out_bits == 0 || out_bits > (nfull - 2) * lifting_size ||
      msg_stride_bytes < (kb * lifting_size + 7) / 8 || out_stride_bytes < (out_bits + 7) / 8) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(launch_ldpc_encode(ctx->d_graphs, (base_graph - 1) * NOF_LIFTING_SIZES + (uint32_t)pos, kb, lifting_size,
                             n_cb, d_msg, msg_stride_bytes, out_bits, d_out, out_stride_bytes,
                             stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

// ================================================================================================================
// OFDM
// ================================================================================================================
extern "C" int nrphy_ofdm_plan_create(nrphy_ctx_t* ctx, const nrphy_ofdm_config_t* cfg, uint32_t nof_ports,
                                      nrphy_ofdm_plan_t** out)
{
  if (ctx == nullptr || cfg == nullptr || out == nullptr || nof_ports == 0 || cfg->numerology > 4 ||
      !dft_size_in_lds(cfg->dft_size) || cfg->dft_size <= 12 * cfg->bw_rb || cfg->bw_rb == 0 || cfg->cp > 1 ||
      !std::isnormal(cfg->scale)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  if (get_twiddle(ctx, cfg->dft_size) == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  nrphy_ofdm_plan* plan = new (std::nothrow) nrphy_ofdm_plan;
  if (plan == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  plan->ctx           = ctx;
  plan->cfg           = *cfg;
  plan->d_twiddle     = get_twiddle(ctx, cfg->dft_size);
  plan->nof_ports     = nof_ports;
  plan->nsymb         = cfg->cp ? 12 : 14; // get_nsymb_per_slot (cyclic_prefix.h:108-114)
  plan->nsym_subframe = plan->nsymb << cfg->numerology;
  plan->slot_stride   = nrphy_ofdm_slot_size(cfg, 0);
  // Phase compensation (TS 38.211 Section 5.4; phase_compensation_lut.h:49-82) times the scale.
  const double        srate = 15000.0 * (double)(1U << cfg->numerology) * (double)cfg->dft_size;
  std::vector<float2> phase(plan->nsym_subframe), phase_rx(plan->nsym_subframe);
  plan->cp.resize(plan->nsym_subframe);
  plan->off.resize(plan->nsym_subframe);
  unsigned offset = 0, in_slot = 0;
  for (unsigned s = 0; s != plan->nsym_subframe; ++s) {
    if (s % plan->nsymb == 0) {
      in_slot = 0;
    }
    const unsigned cp = cp_length(*cfg, s);
    offset += cp;
    const double ph = -2.0 * M_PI * cfg->center_freq_hz * ((double)offset / srate);
    const float  pr = (float)std::cos(ph), pi = (float)std::sin(ph);
    phase[s]        = make_float2(pr * cfg->scale, pi * cfg->scale);
    phase_rx[s]     = make_float2(pr * cfg->scale, -pi * cfg->scale);
    plan->cp[s]     = cp;
    plan->off[s]    = in_slot;
    in_slot += cp + cfg->dft_size;
    offset += cfg->dft_size;
  }
  if (upload(&plan->d_phase, phase.data(), phase.size() * sizeof(float2)) != hipSuccess ||
      upload(&plan->d_phase_rx, phase_rx.data(), phase_rx.size() * sizeof(float2)) != hipSuccess ||
      upload(&plan->d_cp, plan->cp.data(), plan->cp.size() * sizeof(uint32_t)) != hipSuccess ||
      upload(&plan->d_off, plan->off.data(), plan->off.size() * sizeof(uint32_t)) != hipSuccess) {
    nrphy_ofdm_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_plan_destroy(nrphy_ofdm_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  (void)hipSetDevice(plan->ctx->device);
  (void)hipFree(plan->d_phase);
  (void)hipFree(plan->d_phase_rx);
  (void)hipFree(plan->d_cp);
  (void)hipFree(plan->d_off);
  (void)hipFree(plan->d_wire_partials);
  for (auto& kv : plan->d_window_phase) {
    (void)hipFree(kv.second);
  }
  for (hipEvent_t e : plan->events) {
    (void)hipEventDestroy(e);
  }
  delete plan;
  return NRPHY_OK;
}

extern "C" uint32_t nrphy_ofdm_plan_slot_stride(const nrphy_ofdm_plan_t* plan)
{
  return plan ? plan->slot_stride : 0;
}

namespace {

// Amplitude controller parameters as the reference's constructors derive them
// (amplitude_controller_clipping_impl.h:52-62, amplitude_controller_scaling_impl.h).
struct AmplitudeParams {
  float gain, ceiling;
  bool  measure, clip;
};
bool amplitude_params(const nrphy_amplitude_cfg_t& c, AmplitudeParams& a)
{
  if (c.kind > 1) {
    return false;
  }
  a.gain    = std::pow(10.0F, c.input_gain_dB / 20.0F);
  a.ceiling = c.full_scale_lin * std::pow(10.0F, c.ceiling_dBFS / 20.0F);
  a.measure = c.kind == 0;
  a.clip    = c.kind == 0 && c.enable_clipping != 0;
  // a ceiling that is not a normal number cannot be told from the reference's zero-power exception (see the header)
  return std::isfinite(a.gain) && (!a.clip || std::isnormal(a.ceiling));
}

int ofdm_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_grid, const uint32_t* slot_index, void* d_iq,
             const nrphy_iq_wire_cfg_t* wire, nrphy_amplitude_stats_t* d_stats, void* stream)
{
  if (plan == nullptr || d_grid == nullptr || d_iq == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_ctx* ctx = plan->ctx;
  OfdmLaunch p;
  p.window_phase = nullptr;
  p.dft_size    = plan->cfg.dft_size;
  p.rg_size     = 12 * plan->cfg.bw_rb;
  p.nof_ports   = plan->nof_ports;
  p.nsymb       = plan->nsymb;
  p.slot_stride = plan->slot_stride;
  p.twiddle     = plan->d_twiddle;
  p.phase       = plan->d_phase;
  p.cp_len      = plan->d_cp;
  p.sym_offset  = plan->d_off;
#ifdef NRPHY_PROBES
  p.probe = ctx->tune.ofdm_probe; // profiling variant: 1 = drop the IQ stores, 2 = drop the grid loads, 3 = both (outputs are then wrong)
#else
  p.probe = 0;
#endif
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  if (wire != nullptr) {
    AmplitudeParams a;
    if (!amplitude_params(wire->amplitude, a) || !std::isfinite(wire->ci16_scale)) {
      return NRPHY_ERR_ARGUMENT;
    }
    p.wire         = 1;
    p.wire_clip    = a.clip ? 1U : 0U;
    p.wire_gain    = a.gain;
    p.wire_ceiling = a.ceiling;
    p.wire_scale   = wire->ci16_scale;
    // Largest magnitude whose scaled value stays within int16 (so the saturation is an identity below it).
    float sat = wire->ci16_scale != 0.f ? 32767.0f / std::fabs(wire->ci16_scale) : INFINITY;
    while ((double)sat * std::fabs((double)wire->ci16_scale) > 32767.0) {
      sat = std::nextafterf(sat, 0.f);
    }
    // ... squared, and a hair lower: the kernel compares the rounded power re^2 + im^2 of a sample with it
    const float lim = a.clip ? std::fmin(a.ceiling, sat) : sat;
    p.wire_limit    = std::isfinite(lim) ? (float)((double)lim * (double)lim * (1.0 - 1e-6)) : lim;
    p.wire_stats   = a.measure ? d_stats : nullptr;
    if (p.wire_stats != nullptr) {
      // One record per workgroup (at most one workgroup per symbol), added up by a second small kernel.  The buffer belongs to
      // the plan and grows with the largest batch seen (a synchronous reallocation, on growth only): runs of one plan are
      // ordered, as the conventions in mi355_nrphy.h say.
      const size_t need = (size_t)nof_grids * plan->nof_ports * plan->nsymb;
      if (need > plan->wire_partials_cap) {
        if (plan->d_wire_partials != nullptr) {
          HIP_TRY(hipFree(plan->d_wire_partials));
          plan->d_wire_partials   = nullptr;
          plan->wire_partials_cap = 0;
        }
        HIP_TRY(hipMalloc(&plan->d_wire_partials, need * sizeof(uint4)));
        plan->wire_partials_cap = need;
      }
      p.wire_partials = plan->d_wire_partials;
    } else if (d_stats != nullptr) {
      HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(nrphy_amplitude_stats_t) * (size_t)nof_grids * plan->nof_ports, s));
    }
  }
  hipEvent_t* ev = nullptr;
  if (plan->timed_runs < plan->max_timed_runs && plan->timing_counter++ % plan->timing_stride == 0) {
    ev = &plan->events[2 * plan->timed_runs++];
    HIP_TRY(hipEventRecord(ev[0], s));
  }
  HIP_TRY(launch_ofdm(p, nof_grids, (const uint32_t*)d_grid, slot_index, (float2*)d_iq, s));
  if (ev) {
    HIP_TRY(hipEventRecord(ev[1], s));
  }
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ofdm_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_grid,
                              const uint32_t* slot_index, float* d_iq, void* stream)
{
  const TraceRange trace("downlink_baseband");
  return ofdm_run(plan, nof_grids, d_grid, slot_index, d_iq, nullptr, nullptr, stream);
}

extern "C" int nrphy_ofdm_run_ci16(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_grid, const uint32_t* slot_index,
                                   const nrphy_iq_wire_cfg_t* cfg, int16_t* d_iq, nrphy_amplitude_stats_t* d_stats, void* stream)
{
  if (cfg == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const TraceRange trace("downlink_baseband");
  return ofdm_run(plan, nof_grids, d_grid, slot_index, d_iq, cfg, d_stats, stream);
}

// ================================================================================================================
// Lower-PHY tail: amplitude controller, radio sample format, fronthaul compression
// ================================================================================================================
extern "C" int nrphy_amplitude_control(nrphy_ctx_t* ctx, const nrphy_amplitude_cfg_t* cfg, uint32_t n_buffers, uint32_t nof_samples,
                                       const float* d_in, size_t in_stride, float* d_out, size_t out_stride,
                                       nrphy_amplitude_stats_t* d_stats, void* stream)
{
  AmplitudeParams a;
  if (ctx == nullptr || cfg == nullptr || d_in == nullptr || d_out == nullptr || !amplitude_params(*cfg, a) ||
      (n_buffers > 1 && (in_stride < nof_samples || out_stride < nof_samples))) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  if (d_stats != nullptr) {
    HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(nrphy_amplitude_stats_t) * (size_t)n_buffers, s));
  }
  for (uint32_t first = 0; first < n_buffers; first += 32768) { // the launch's second grid dimension holds 65535
    AmplitudeLaunch p;
    p.in          = d_in + 2 * first * in_stride;
    p.out         = d_out + 2 * first * out_stride;
    p.in_stride   = in_stride;
    p.out_stride  = out_stride;
    p.nof_samples = nof_samples;
    p.measure     = a.measure ? 1U : 0U;
    p.clip        = a.clip ? 1U : 0U;
    p.gain        = a.gain;
    p.ceiling     = a.ceiling;
    p.stats       = d_stats ? d_stats + first : nullptr;
    HIP_TRY(launch_amplitude(p, std::min<uint32_t>(32768, n_buffers - first), s));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_amplitude_metrics(const nrphy_amplitude_cfg_t* cfg, const nrphy_amplitude_stats_t* stats,
                                       nrphy_amplitude_metrics_t* m)
{
  if (cfg == nullptr || stats == nullptr || m == nullptr || cfg->kind > 1) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (cfg->kind == 1) { // amplitude_controller_scaling_impl returns empty metrics
    std::memset(m, 0, sizeof(*m));
    return NRPHY_OK;
  }
  // amplitude_controller_clipping_impl::process, the part after the vector operations
  const float full_scale_pwr = cfg->full_scale_lin * cfg->full_scale_lin;
  const float avg            = stats->nof_samples ? stats->sum_power / (float)stats->nof_samples : 0.0F;
  m->clipping_enabled        = cfg->enable_clipping ? 1U : 0U;
  m->gain_dB                 = 20.0F * std::log10(std::pow(10.0F, cfg->input_gain_dB / 20.0F)); // convert_amplitude_to_dB
  m->avg_power_fs            = avg / full_scale_pwr;
  m->peak_power_fs           = stats->peak_power / full_scale_pwr;
  if (!std::isnormal(avg) || !std::isnormal(stats->peak_power)) {
    m->papr_lin = 1.0F;
    return NRPHY_OK;
  }
  m->papr_lin = stats->peak_power / avg;
  if (cfg->enable_clipping) {
    m->nof_processed_samples += stats->nof_samples;
    m->nof_clipped_samples += stats->nof_clipped;
    m->clipping_probability = (double)m->nof_clipped_samples / (double)m->nof_processed_samples;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_amplitude_control_host(nrphy_ctx_t* ctx, const nrphy_amplitude_cfg_t* cfg, const float* in,
                                            uint32_t nof_samples, float* out, nrphy_amplitude_metrics_t* metrics)
{
  if (ctx == nullptr || cfg == nullptr || in == nullptr || out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall     call(ctx);
  const size_t bytes = (size_t)nof_samples * sizeof(float2);
  float*       d_buf = call.mem<float>(SCRATCH_IQ, bytes + 64);
  if (d_buf == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  nrphy_amplitude_stats_t* d_stats = (nrphy_amplitude_stats_t*)((uint8_t*)d_buf + ((bytes + 15) & ~(size_t)15));
  HIP_TRY(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_amplitude_control(ctx, cfg, 1, nof_samples, d_buf, nof_samples, d_buf, nof_samples, d_stats, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  nrphy_amplitude_stats_t st;
  HIP_TRY(hipMemcpyAsync(out, d_buf, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(&st, d_stats, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return metrics ? nrphy_amplitude_metrics(cfg, &st, metrics) : NRPHY_OK;
}

extern "C" int nrphy_iq_convert_ci16(nrphy_ctx_t* ctx, uint32_t n_buffers, uint32_t nof_samples, const float* d_in, size_t in_stride,
                                     float scale, int16_t* d_out, size_t out_stride, void* stream)
{
  if (ctx == nullptr || d_in == nullptr || d_out == nullptr || !std::isfinite(scale) ||
      (n_buffers > 1 && (in_stride < nof_samples || out_stride < nof_samples))) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  for (uint32_t first = 0; first < n_buffers; first += 32768) {
    HIP_TRY(launch_convert_ci16(d_in + 2 * first * in_stride, in_stride, d_out + 2 * first * out_stride, out_stride,
                                std::min<uint32_t>(32768, n_buffers - first), nof_samples, scale, s));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_iq_convert_ci16_host(nrphy_ctx_t* ctx, const float* in, uint32_t nof_samples, float scale, int16_t* out)
{
  if (ctx == nullptr || in == nullptr || out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall     call(ctx);
  const size_t bytes = (size_t)nof_samples * sizeof(float2), obytes = (size_t)nof_samples * 4;
  uint8_t*     d_buf = call.mem<uint8_t>(SCRATCH_IQ, bytes + obytes + 64);
  if (d_buf == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  int16_t* d_out = (int16_t*)(d_buf + ((bytes + 15) & ~(size_t)15));
  HIP_TRY(hipMemcpyAsync(d_buf, in, bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_iq_convert_ci16(ctx, 1, nof_samples, (const float*)d_buf, nof_samples, scale, d_out, nof_samples, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(out, d_out, obytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" uint32_t nrphy_ofh_compressed_prb_bytes(const nrphy_ofh_compression_cfg_t* cfg)
{
  return cfg ? 3U * cfg->data_width + (cfg->type == 1 ? 1U : 0U) : 0U;
}

extern "C" int nrphy_ofh_compress(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t n_rows, uint32_t nof_prb,
                                  const void* d_prbs, size_t row_stride, uint8_t* d_out, size_t out_row_stride, void* stream)
{
  // Below 8 bits the reference's packer has no defined result (it hands bit_buffer::insert values wider than the
  // field, compressed_prb_packer.cpp:39-47).
  if (ctx == nullptr || cfg == nullptr || d_prbs == nullptr || d_out == nullptr || cfg->type > 1 || cfg->data_width < 8 ||
      cfg->data_width > 16 || !std::isfinite(cfg->iq_scaling) || nof_prb > NRPHY_MAX_RB ||
      (n_rows > 1 && (row_stride < 12 * (size_t)nof_prb || out_row_stride < (size_t)nof_prb * nrphy_ofh_compressed_prb_bytes(cfg)))) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  for (uint32_t first = 0; first < n_rows; first += 32768) {
    OfhCompressLaunch p;
    p.prbs           = (const uint32_t*)d_prbs + first * row_stride;
    p.out            = d_out + first * out_row_stride;
    p.row_stride     = row_stride;
    p.out_row_stride = out_row_stride;
    p.nof_prb        = nof_prb;
    p.data_width     = cfg->data_width;
    p.bfp            = cfg->type == 1 ? 1U : 0U;
    // the AVX2 compressors convert the whole call at once for BFP and for the widths their packer has (9, 16)
    p.whole_span = (cfg->type == 1 || cfg->data_width == 9 || cfg->data_width == 16) ? 1U : 0U;
    // quantizer: gain = 2^(width - 1) - 1, 16 bits for BFP (Q_BIT_WIDTH); scale = gain * iq_scaling in float
    const float gain = (float)((1 << ((cfg->type == 1 ? 16 : (int)cfg->data_width) - 1)) - 1.0F);
    p.scale          = gain * cfg->iq_scaling;
    HIP_TRY(launch_ofh_compress(p, std::min<uint32_t>(32768, n_rows - first), s));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ofh_compress_host(nrphy_ctx_t* ctx, const nrphy_ofh_compression_cfg_t* cfg, uint32_t nof_prb, const void* prbs,
                                       uint8_t* out)
{
  if (ctx == nullptr || cfg == nullptr || prbs == nullptr || out == nullptr || nof_prb == 0 || nof_prb > NRPHY_MAX_RB) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall     call(ctx);
  const size_t in_bytes = (size_t)nof_prb * 48, out_bytes = (size_t)nof_prb * 49;
  uint8_t*     d_buf    = call.mem<uint8_t>(SCRATCH_GRID, in_bytes + out_bytes + 64);
  if (d_buf == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  uint8_t* d_out = d_buf + ((in_bytes + 15) & ~(size_t)15);
  HIP_TRY(hipMemcpyAsync(d_buf, prbs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  const int rc = nrphy_ofh_compress(ctx, cfg, 1, nof_prb, d_buf, 12 * (size_t)nof_prb, d_out, out_bytes, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)nof_prb * nrphy_ofh_compressed_prb_bytes(cfg), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_demod_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const float* d_iq,
                                    const uint32_t* slot_index, uint32_t window_offset, void* d_grid, void* stream)
{
  // ofdm_demodulator_impl.cpp:58-63: the window offset must stay inside the shortest cyclic prefix.
  if (plan == nullptr || d_grid == nullptr || d_iq == nullptr ||
      window_offset >= (144U * plan->cfg.dft_size) / 2048U) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_ctx* ctx = plan->ctx;
  OfdmLaunch p;
  p.window_phase = nullptr;
  p.dft_size    = plan->cfg.dft_size;
  p.rg_size     = 12 * plan->cfg.bw_rb;
  p.nof_ports   = plan->nof_ports;
  p.nsymb       = plan->nsymb;
  p.slot_stride = plan->slot_stride;
  p.twiddle     = plan->d_twiddle;
  p.phase       = plan->d_phase_rx;
  p.cp_len      = plan->d_cp;
  p.sym_offset  = plan->d_off;
  p.probe       = 0;
  p.window_phase = nullptr;
  if (window_offset != 0) {
    // The reference rotates bin i by std::polar(1.0F, omega * i) with omega = offset * 2 pi / N rounded to float
    // (ofdm_demodulator_impl.cpp:68-76): omega * i reaches hundreds of radians, so its float rounding shows in the
    // output (1e-5 of the largest bin); the table is built here with the same arithmetic instead of exactly.
    std::lock_guard<std::mutex> lock(plan->window_mutex);
    auto                        it = plan->d_window_phase.find(window_offset);
    if (it == plan->d_window_phase.end()) {
      const unsigned      n = plan->cfg.dft_size;
      std::vector<float2> w(n);
      const float         omega = static_cast<float>(window_offset) * static_cast<float>(2.0 * M_PI) / static_cast<float>(n);
      for (unsigned i = 0; i != n; ++i) {
        const std::complex<float> v = std::polar(1.0F, omega * static_cast<float>(i));
        w[i]                        = make_float2(v.real(), v.imag());
      }
      float2* d_w = nullptr;
      HIP_TRY(hipSetDevice(ctx->device));
      if (upload(&d_w, w.data(), w.size() * sizeof(float2)) != hipSuccess) {
        return NRPHY_ERR_DEVICE;
      }
      it = plan->d_window_phase.emplace(window_offset, d_w).first;
    }
    p.window_phase = it->second;
  }
  HIP_TRY(launch_ofdm_demod(p, nof_grids, (const float2*)d_iq, slot_index, window_offset, (uint32_t*)d_grid,
                            stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_demodulate_slot_host(nrphy_ofdm_plan_t* plan, const float* iq, uint32_t slot_index,
                                               uint32_t window_offset, void* grid)
{
  if (plan == nullptr || iq == nullptr || grid == nullptr || slot_index >= (1U << plan->cfg.numerology)) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_ctx*   ctx        = plan->ctx;
  HostCall     call(ctx);
  const size_t grid_words = (size_t)plan->nof_ports * NRPHY_NSYMB * 12 * plan->cfg.bw_rb;
  const size_t slot_size  = nrphy_ofdm_slot_size(&plan->cfg, slot_index);
  uint32_t*    d_grid     = call.mem<uint32_t>(SCRATCH_GRID, grid_words * 4);
  float2*      d_iq       = call.mem<float2>(SCRATCH_IQ, (size_t)plan->nof_ports * plan->slot_stride * sizeof(float2));
  uint32_t*    d_slot     = call.mem<uint32_t>(SCRATCH_SMALL, 16);
  if (d_grid == nullptr || d_iq == nullptr || d_slot == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d_slot, &slot_index, sizeof(slot_index), hipMemcpyHostToDevice));
  // Host: ports back to back, slot_size samples each; device: slot_stride apart.
  HIP_TRY(hipMemcpy2D(d_iq, (size_t)plan->slot_stride * sizeof(float2), iq, slot_size * sizeof(float2),
                      slot_size * sizeof(float2), plan->nof_ports, hipMemcpyHostToDevice));
  const int rc = nrphy_ofdm_demod_run(plan, 1, (const float*)d_iq, d_slot, window_offset, d_grid, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  // Only the symbols a slot has (12 with extended cyclic prefix) are written, as by the reference's demodulator.
  const size_t port_bytes = (size_t)NRPHY_NSYMB * 12 * plan->cfg.bw_rb * 4;
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy2D(grid, port_bytes, d_grid, port_bytes, (size_t)plan->nsymb * 12 * plan->cfg.bw_rb * 4, plan->nof_ports,
                      hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_demodulate_symbol_host(nrphy_ofdm_plan_t* plan, const float* input, uint32_t input_size,
                                                 uint32_t symbol_index, uint32_t window_offset, void* grid_row)
{
  if (plan == nullptr || input == nullptr || grid_row == nullptr || symbol_index >= plan->nsym_subframe ||
      input_size != plan->cp[symbol_index] + plan->cfg.dft_size) { // ofdm_demodulator_impl.cpp:110-118
    return NRPHY_ERR_ARGUMENT;
  }
  // One symbol of one port: the samples are placed where the slot kernel expects them (the other symbols of the
  // staging slot transform zeros), the symbol's row is read back.
  nrphy_ctx*     ctx  = plan->ctx;
  HostCall       call(ctx);
  const uint32_t rg   = 12 * plan->cfg.bw_rb;
  const uint32_t slot = symbol_index / plan->nsymb, l = symbol_index % plan->nsymb;
  const size_t   iq_samples = (size_t)plan->nof_ports * plan->slot_stride;
  uint32_t*      d_grid     = call.mem<uint32_t>(SCRATCH_GRID, (size_t)plan->nof_ports * NRPHY_NSYMB * rg * 4);
  float2*        d_iq       = call.mem<float2>(SCRATCH_IQ, iq_samples * sizeof(float2));
  uint32_t*      d_slot     = call.mem<uint32_t>(SCRATCH_SMALL, 16);
  if (d_grid == nullptr || d_iq == nullptr || d_slot == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemset(d_iq, 0, iq_samples * sizeof(float2)));
  HIP_TRY(hipMemcpy(d_iq + plan->off[symbol_index], input, (size_t)input_size * sizeof(float2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_slot, &slot, sizeof(slot), hipMemcpyHostToDevice));
  const int rc = nrphy_ofdm_demod_run(plan, 1, (const float*)d_iq, d_slot, window_offset, d_grid, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(grid_row, d_grid + (size_t)l * rg, (size_t)rg * 4, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_plan_enable_timing(nrphy_ofdm_plan_t* plan, uint32_t max_runs)
{
  if (plan == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (hipEvent_t e : plan->events) {
    (void)hipEventDestroy(e);
  }
  plan->events.assign(2 * (size_t)max_runs, nullptr);
  for (hipEvent_t& e : plan->events) {
    HIP_TRY(hipEventCreate(&e));
  }
  plan->max_timed_runs = max_runs;
  plan->timed_runs     = 0;
  plan->timing_counter = 0;
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_plan_timing_stride(nrphy_ofdm_plan_t* plan, uint32_t stride)
{
  if (plan == nullptr || stride == 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  plan->timing_stride  = stride;
  plan->timing_counter = 0;
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_plan_kernel_time(nrphy_ofdm_plan_t* plan, float* avg_ms, uint32_t* nof_runs)
{
  if (plan == nullptr || avg_ms == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  double sum = 0;
  for (uint32_t r = 0; r != plan->timed_runs; ++r) {
    HIP_TRY(hipEventSynchronize(plan->events[2 * r + 1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, plan->events[2 * r], plan->events[2 * r + 1]));
    sum += ms;
  }
  *avg_ms = plan->timed_runs ? (float)(sum / plan->timed_runs) : 0.f;
  if (nof_runs) {
    *nof_runs = plan->timed_runs;
  }
  plan->timed_runs = 0;
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_modulate_symbol_host(nrphy_ofdm_plan_t* plan, const void* grid, uint32_t port_index,
                                               uint32_t symbol_index, float* output, uint32_t output_size)
{
  if (plan == nullptr || grid == nullptr || output == nullptr || port_index >= plan->nof_ports ||
      symbol_index >= plan->nsym_subframe ||
      output_size != plan->cp[symbol_index] + plan->cfg.dft_size) { // ofdm_modulator_impl.cpp:68-75
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_ctx*     ctx        = plan->ctx;
  HostCall       call(ctx);
  const size_t   grid_words = (size_t)plan->nof_ports * NRPHY_NSYMB * 12 * plan->cfg.bw_rb;
  const size_t   iq_samples = (size_t)plan->nof_ports * plan->slot_stride;
  const uint32_t slot       = symbol_index / plan->nsymb;
  uint32_t*      d_grid     = call.mem<uint32_t>(SCRATCH_GRID, grid_words * 4);
  float2*        d_iq       = call.mem<float2>(SCRATCH_IQ, iq_samples * sizeof(float2));
  uint32_t*      d_slot     = call.mem<uint32_t>(SCRATCH_SMALL, 16);
  if (d_grid == nullptr || d_iq == nullptr || d_slot == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d_grid, grid, grid_words * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_slot, &slot, sizeof(slot), hipMemcpyHostToDevice));
  const int rc = nrphy_ofdm_run(plan, 1, d_grid, d_slot, (float*)d_iq, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  const size_t src = (size_t)port_index * plan->slot_stride + plan->off[symbol_index];
  HIP_TRY(hipMemcpy(output, d_iq + src, (size_t)output_size * sizeof(float2), hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

extern "C" int nrphy_dft_run(nrphy_ctx_t* ctx, uint32_t size, int inverse, uint32_t batch, const float* d_in,
                             float* d_out, void* stream)
{
  if (ctx == nullptr || d_in == nullptr || d_out == nullptr || !dft_size_supported(size)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t   s  = stream ? (hipStream_t)stream : ctx->stream;
  uint32_t      n1 = 1, n2 = size;
  dft_split(size, &n1, &n2);
  const float2* tw    = get_twiddle(ctx, size);
  const float2* tw_n2 = (n1 == 1) ? tw : get_twiddle(ctx, n2);
  if (tw == nullptr || tw_n2 == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  // The sizes beyond 6144 take two passes through a scratch copy of the batch (stream-ordered allocation).
  StreamStaging staging(s);
  float2*       d_tmp = nullptr;
  if (n1 != 1 && batch != 0) {
    d_tmp = (float2*)staging.alloc((size_t)batch * size * sizeof(float2));
    if (d_tmp == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  HIP_TRY(launch_dft(size, inverse, batch, tw, tw_n2, d_tmp, (const float2*)d_in, (float2*)d_out, s));
  return NRPHY_OK;
}

extern "C" int nrphy_dft_run_host(nrphy_ctx_t* ctx, uint32_t size, int inverse, const float* in, float* out)
{
  if (ctx == nullptr || in == nullptr || out == nullptr || !dft_size_supported(size)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t bytes = (size_t)size * sizeof(float2);
  HostCall     call(ctx);
  uint8_t*     d[2]; // in, out
  if (!call.carve(SCRATCH_IQ, {bytes, bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], in, bytes, hipMemcpyHostToDevice));
  const int rc = nrphy_dft_run(ctx, size, inverse, 1, (const float*)d[0], (float*)d[1], ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(out, d[1], bytes, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

extern "C" int nrphy_ofdm_modulate_slot_host(nrphy_ofdm_plan_t* plan, const void* grid, uint32_t slot_index, float* iq)
{
  if (plan == nullptr || grid == nullptr || iq == nullptr || slot_index >= (1U << plan->cfg.numerology)) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_ctx*     ctx        = plan->ctx;
  HostCall       call(ctx);
  const size_t   grid_words = (size_t)plan->nof_ports * NRPHY_NSYMB * 12 * plan->cfg.bw_rb;
  const size_t   iq_samples = (size_t)plan->nof_ports * plan->slot_stride;
  const uint32_t slot_size  = nrphy_ofdm_slot_size(&plan->cfg, slot_index);
  uint32_t*      d_grid     = call.mem<uint32_t>(SCRATCH_GRID, grid_words * 4);
  float2*        d_iq       = call.mem<float2>(SCRATCH_IQ, iq_samples * sizeof(float2));
  uint32_t*      d_slot     = call.mem<uint32_t>(SCRATCH_SMALL, 16);
  if (d_grid == nullptr || d_iq == nullptr || d_slot == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d_grid, grid, grid_words * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_slot, &slot_index, sizeof(slot_index), hipMemcpyHostToDevice));
  const int rc = nrphy_ofdm_run(plan, 1, d_grid, d_slot, (float*)d_iq, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  // Ports back to back on the host, slot_stride apart on the device: one strided copy.
  HIP_TRY(hipMemcpy2D(iq, (size_t)slot_size * sizeof(float2), d_iq, (size_t)plan->slot_stride * sizeof(float2),
                      (size_t)slot_size * sizeof(float2), plan->nof_ports, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}
