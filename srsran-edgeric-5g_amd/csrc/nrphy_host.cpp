// Host side of libmi355nrphy.so: the C ABI of include/mi355_nrphy.h.
//
// This file is the context and what it owns: the lifted graphs, the TB-CRC and Gold tables, the twiddle tables, the tunables.
// Every seam's host code lives next to its kernels (X_kernels.hip / X.hip -> X_host.cpp).  No compute happens on the host and
// there is no CPU fallback: every entry point that produces PHY output needs a HIP device.
#include "ldpc_base_graph_host.h"
#include "nrphy_host_internal.h"
#include "nrphy_trace.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

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
  return dft_size_supported(size) ? get_twiddle_table(ctx, size) : nullptr;
}

const float2* get_twiddle_table(nrphy_ctx* ctx, uint32_t size)
{
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
