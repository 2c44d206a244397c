// Host side of the UCI decoder (uci_kernels.hip): validation -- what short_block_detector_impl::detect and polar_code_impl::set
// assert on, after the segmentation rule of R/include/srsran/ran/uci/uci_info.h -- and, per distinct polar code (K, E) of a plan,
// the uplink construction (n_max = 10, parity-check bits; polar_code_impl::set, R/lib/phy/upper/channel_coding/polar/
// polar_code_impl.cpp:421-490), the channel de-interleaver's permutation, the de-allocator's positions, the CRC weights and the
// decoder's walk over the tree flattened into a list of operations (polar_decoder_impl::simplified_node).
#include "nrphy_host_internal.h"
#include "pusch_select_host.h"

namespace {

#include "nr_polar_tables.inc"

// TS 38.212 Table 5.4.1.1-1.
const uint8_t SUBBLOCK_PATTERN[32] = NR_POLAR_SUBBLOCK_PATTERN;

const CrcField CRC6_FIELD  = {0x61U, 6};
const CrcField CRC11_FIELD = {0xE21U, 11};

uint32_t nof_codeblocks(uint32_t A, uint32_t E) // get_nof_uci_codeblocks
{
  return ((A >= 360 && E >= 1088) || A >= 1013) ? 2 : 1;
}
uint32_t crc_size(uint32_t A) // get_uci_crc_size
{
  return A < 12 ? 0 : (A < 20 ? 6 : 11);
}
bool bits_per_symbol(uint32_t modulation, uint32_t* bps)
{
  switch (modulation) {
    case NRPHY_MOD_PI2_BPSK:
    case NRPHY_MOD_BPSK:
      *bps = 1;
      return true;
    case NRPHY_MOD_QPSK:
    case NRPHY_MOD_QAM16:
    case NRPHY_MOD_QAM64:
    case NRPHY_MOD_QAM256:
      *bps = modulation;
      return true;
    default:
      return false;
  }
}

// The uplink polar code of one block.
struct UciPolarCode {
  uint32_t              n = 0, N = 0, mode = 0, nof_pc = 0;
  std::vector<uint8_t>  info_mask; // K + nPC positions that are not frozen
  std::vector<uint16_t> info_pos;  // the K of them that carry block bits, ascending (the de-allocator's order)
  std::vector<uint16_t> pc_pos;    // parity-check positions, ascending
};

// polar_code_impl::set(K, E, 10, ...).  False for what set_code_params asserts on.
bool build_uci_polar_code(uint32_t K, uint32_t E, UciPolarCode& code)
{
  if (K < 18 || (K > 25 && K < 31) || K > 1023 || E > 8192) {
    return false;
  }
  const uint32_t nPC = K <= 25 ? 3 : 0, nWmPC = (K <= 25 && E > K + 189) ? 1 : 0;
  if (K + nPC >= E) {
    return false;
  }
  uint32_t e = 1, k = 0;
  while ((1U << e) < E) {
    ++e;
  }
  while ((1U << k) < K) {
    ++k;
  }
  const uint32_t n1 = (8 * E <= 9 * (1U << (e - 1)) && 16 * K < 9 * E) ? e - 1 : e;
  const uint32_t n  = std::max<uint32_t>(5, std::min<uint32_t>(std::min(n1, k + 3), 10));
  const uint32_t N  = 1U << n;
  if (K >= N) {
    return false;
  }
  auto J = [N](uint32_t i) { return SUBBLOCK_PATTERN[(32 * i) / N] * (N / 32) + i % (N / 32); };
  std::vector<uint8_t> barred(N, 0);
  code.mode = 0;
  if (N > E) {
    uint32_t T = 0;
    if (16 * K <= 7 * E) {
      code.mode = 1;
      T         = (E >= 3 * N / 4) ? 3 * N / 4 - (E >> 1) - 1 : 9 * N / 16 - (E >> 2);
      for (uint32_t i = 0; i != N - E; ++i) {
        barred[J(i)] = 1;
      }
    } else {
      code.mode = 2;
      for (uint32_t i = E; i != N; ++i) {
        barred[J(i)] = 1;
      }
    }
    for (uint32_t i = 0; i <= T; ++i) {
      barred[i] = 1;
    }
  }
  // The K + nPC most reliable of what is left, least reliable first.
  std::vector<uint16_t> k_set;
  for (int i = 1023; i >= 0 && k_set.size() != K + nPC; --i) {
    const uint32_t q = NR_POLAR_RELIABILITY[i];
    if (q < N && !barred[q]) {
      k_set.push_back((uint16_t)q);
    }
  }
  if (k_set.size() != K + nPC) {
    return false;
  }
  std::reverse(k_set.begin(), k_set.end());
  // Parity-check positions: the nPC - nWmPC least reliable, and with nWmPC the fixed position the reference uses.
  std::vector<uint16_t> pc;
  for (uint32_t i = 0; i != nPC - nWmPC; ++i) {
    pc.push_back(k_set[i]);
  }
  if (nWmPC == 1) {
    pc.push_back(K <= 21 ? 252 : 248);
  }
  std::sort(pc.begin(), pc.end());
  pc.push_back(1024); // the end mark
  code.n      = n;
  code.N      = N;
  code.nof_pc = nPC;
  code.info_mask.assign(N, 0);
  for (uint16_t q : k_set) {
    code.info_mask[q] = 1;
  }
  // polar_deallocator_impl::deallocate: ascending over the set, a position equal to the next parity-check one is skipped.
  code.info_pos.clear();
  code.pc_pos.assign(pc.begin(), pc.end() - 1);
  uint32_t i_pc = 0;
  for (uint32_t i = 0; i != N; ++i) {
    if (!code.info_mask[i]) {
      continue;
    }
    if (i == pc[i_pc]) {
      ++i_pc;
    } else {
      code.info_pos.push_back((uint16_t)i);
    }
  }
  return code.info_pos.size() == K; // otherwise the reference writes past its buffer: refused here
}

// polar_decoder_impl: node types from the frozen set (tmp_node_s::compute), then simplified_node's recursion written out.  A
// node that ends at N is nobody's left child: its partial sums are never read, so its XOR is left out (the reference returns
// before it, flag_finished).
struct TreeWalk {
  uint32_t                          n;
  std::vector<std::vector<uint8_t>> type; // [stage][node]: 0 rate-0, 2 rate-R, 3 rate-1
  std::vector<uint32_t>             ops;
  void node(uint32_t s, uint32_t pos)
  {
    const uint8_t t = type[s][pos >> s];
    if (t == 0) {
      return;
    }
    if (t == 3) {
      ops.push_back(UCI_OP_RATE1 | (s << 2) | (pos << 6));
      return;
    }
    const uint32_t h = 1U << (s - 1);
    ops.push_back(UCI_OP_F | (s << 2) | (pos << 6));
    node(s - 1, pos);
    ops.push_back(UCI_OP_G | (s << 2) | (pos << 6));
    node(s - 1, pos + h);
    if (pos + 2 * h != (1U << n)) {
      ops.push_back(UCI_OP_XOR | (s << 2) | (pos << 6));
    }
  }
};

std::vector<uint32_t> tree_walk(const UciPolarCode& code)
{
  TreeWalk w;
  w.n = code.n;
  w.type.resize(code.n + 1);
  std::vector<uint8_t> not0(code.info_mask), is1(code.info_mask);
  w.type[0].resize(code.N);
  for (uint32_t j = 0; j != code.N; ++j) {
    w.type[0][j] = (uint8_t)(3 * not0[j]);
  }
  for (uint32_t s = 1; s <= code.n; ++s) {
    const uint32_t size = code.N >> s;
    w.type[s].resize(size);
    for (uint32_t j = 0; j != size; ++j) {
      not0[j]      = not0[2 * j] | not0[2 * j + 1];
      is1[j]       = is1[2 * j] & is1[2 * j + 1];
      w.type[s][j] = (uint8_t)(2 * not0[j] + is1[j]);
    }
  }
  w.node(code.n, 0);
  return w.ops;
}

// ch_interleaver_rm_rx_c: position i_in of the de-interleaved block comes from input position i_out.
std::vector<uint16_t> channel_deinterleaver(uint32_t E)
{
  uint32_t S = 1, T = 1;
  while (S < E) {
    S += ++T;
  }
  std::vector<uint16_t> ch(E, 0);
  uint32_t              i_out = 0;
  for (uint32_t r = 0; r != T; ++r) {
    uint32_t i_in = r;
    for (uint32_t c = 0; c != T - r && i_in < E; ++c) {
      ch[i_in] = (uint16_t)i_out++;
      i_in += T - c;
    }
  }
  return ch;
}

struct BlockSizes {
  uint32_t C, L, K, E;
};
BlockSizes block_sizes(uint32_t A, uint32_t E)
{
  BlockSizes b;
  b.C = nof_codeblocks(A, E);
  b.L = crc_size(A);
  b.K = (A + b.C - 1) / b.C + b.L; // A / C message bits and A % C filler bits, or ceil(A / C) message bits: the same
  b.E = E / b.C;
  return b;
}

int validate(const nrphy_uci_decoder_cfg_t* c)
{
  if (c == nullptr || c->message_length < 1 || c->message_length > 1706) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c->message_length <= 2) {
    uint32_t bps = 0;
    return bits_per_symbol(c->modulation, &bps) && c->llr_length >= bps ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
  }
  if (c->message_length <= 11) {
    return c->llr_length > c->message_length ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
  }
  const BlockSizes b = block_sizes(c->message_length, c->llr_length);
  UciPolarCode     code;
  return build_uci_polar_code(b.K, b.E, code) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

} // namespace

struct nrphy_uci_decoder_plan {
  nrphy_ctx*   ctx     = nullptr;
  uint32_t     n       = 0;
  void*        d_arena = nullptr;
  UciMsgDesc*  d_msg   = nullptr;
  UciCodeDesc* d_code  = nullptr;
  uint16_t*    d_tab16 = nullptr;
  uint32_t*    d_ops   = nullptr;
  bool         selects = false; // some message names a select word
};

extern "C" int nrphy_uci_decoder_validate(const nrphy_uci_decoder_cfg_t* cfg)
{
  return validate(cfg);
}

extern "C" int nrphy_uci_decoder_plan_destroy(nrphy_uci_decoder_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  if (plan->d_arena != nullptr) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena);
  }
  delete plan;
  return NRPHY_OK;
}

int uci_decoder_plan_create_select(nrphy_ctx_t* ctx, uint32_t n, const nrphy_uci_decoder_cfg_t* cfgs, const uint64_t* llr_offset,
                                   const uint64_t* message_offset, const uint32_t* select_word, const uint32_t* select_value,
                                   nrphy_uci_decoder_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || llr_offset == nullptr || message_offset == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<UciMsgDesc>      msg(n);
  std::vector<UciCodeDesc>     codes;
  std::vector<uint16_t>        tab16;
  std::vector<uint32_t>        ops;
  std::map<uint64_t, uint32_t> code_index; // (K, E) -> index: each distinct code is built once
  bool                         selects = false;
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_uci_decoder_cfg_t& c = cfgs[i];
    if (validate(&c) != NRPHY_OK) {
      return NRPHY_ERR_ARGUMENT;
    }
    UciMsgDesc& m = msg[i];
    std::memset(&m, 0, sizeof(m));
    m.A              = c.message_length;
    m.E              = c.llr_length;
    m.code           = UCI_NO_CODE;
    m.nof_blocks     = 1;
    m.llr_offset     = llr_offset[i];
    m.message_offset = message_offset[i];
    m.select_word    = select_word != nullptr && select_value != nullptr ? select_word[i] : NO_SELECT_WORD;
    m.select_value   = m.select_word != NO_SELECT_WORD ? select_value[i] : 0;
    selects          = selects || m.select_word != NO_SELECT_WORD;
    if (c.message_length <= 2) {
      bits_per_symbol(c.modulation, &m.bps);
    }
    if (c.message_length <= 11) {
      continue;
    }
    const BlockSizes b   = block_sizes(c.message_length, c.llr_length);
    const uint64_t   key = ((uint64_t)b.K << 32) | b.E;
    m.nof_blocks         = b.C;
    auto it              = code_index.find(key);
    if (it == code_index.end()) {
      UciPolarCode code;
      if (!build_uci_polar_code(b.K, b.E, code)) {
        return NRPHY_ERR_ARGUMENT;
      }
      UciCodeDesc d;
      std::memset(&d, 0, sizeof(d));
      d.n        = code.n;
      d.K        = b.K;
      d.E        = b.E;
      d.mode     = code.mode;
      d.crc_size = b.L;
      const std::vector<uint32_t> walk = tree_walk(code);
      d.nof_ops                        = (uint32_t)walk.size();
      d.ops_offset                     = (uint32_t)ops.size();
      ops.insert(ops.end(), walk.begin(), walk.end());
      const std::vector<uint16_t> ch = channel_deinterleaver(b.E);
      d.ch_offset                    = (uint32_t)tab16.size();
      tab16.insert(tab16.end(), ch.begin(), ch.end());
      d.info_offset = (uint32_t)tab16.size();
      tab16.insert(tab16.end(), code.info_pos.begin(), code.info_pos.end());
      d.crc_offset       = (uint32_t)tab16.size();
      const CrcField& f  = b.L == 11 ? CRC11_FIELD : CRC6_FIELD;
      for (uint32_t k = 0; k != b.K; ++k) {
        tab16.push_back((uint16_t)f.xpow((int64_t)(b.K - 1 - k)));
      }
      it = code_index.emplace(key, (uint32_t)codes.size()).first;
      codes.push_back(d);
    }
    m.code = it->second;
  }
  auto* plan = new nrphy_uci_decoder_plan;
  plan->ctx  = ctx;
  plan->n    = n;
  plan->selects = selects;
  DeviceArena arena;
  arena.add(&plan->d_msg, msg.data(), msg.size() * sizeof(UciMsgDesc));
  arena.add(&plan->d_code, codes.data(), codes.size() * sizeof(UciCodeDesc));
  arena.add(&plan->d_tab16, tab16.data(), tab16.size() * sizeof(uint16_t));
  arena.add(&plan->d_ops, ops.data(), ops.size() * sizeof(uint32_t));
  void* unused = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_uci_decoder_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_uci_decoder_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_uci_decoder_cfg_t* cfgs,
                                             const uint64_t* llr_offset, const uint64_t* message_offset,
                                             nrphy_uci_decoder_plan_t** out)
{
  return uci_decoder_plan_create_select(ctx, n, cfgs, llr_offset, message_offset, nullptr, nullptr, out);
}

int uci_decoder_run_select(nrphy_uci_decoder_plan_t* plan, const int8_t* d_llr, uint8_t* d_message, uint32_t* d_status,
                           const uint32_t* d_select, void* stream)
{
  if (plan == nullptr || d_llr == nullptr || d_message == nullptr || d_status == nullptr || ((uintptr_t)d_status & 3U) != 0 ||
      (plan->selects && d_select == nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  UciLaunch p;
  p.select  = plan->selects ? d_select : nullptr;
  p.msg     = plan->d_msg;
  p.code    = plan->d_code;
  p.tab16   = plan->d_tab16;
  p.ops     = plan->d_ops;
  p.llr     = d_llr;
  p.message = d_message;
  p.status  = d_status;
  p.n       = plan->n;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_uci_decoder(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_uci_decoder_run(nrphy_uci_decoder_plan_t* plan, const int8_t* d_llr, uint8_t* d_message, uint32_t* d_status,
                                     void* stream)
{
  return uci_decoder_run_select(plan, d_llr, d_message, d_status, nullptr, stream);
}

extern "C" int nrphy_uci_decode_host(nrphy_ctx_t* ctx, const nrphy_uci_decoder_cfg_t* cfg, const int8_t* llr, uint8_t* message,
                                     uint32_t* status)
{
  if (ctx == nullptr || llr == nullptr || message == nullptr || status == nullptr || validate(cfg) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  HostCall call(ctx);
  uint8_t* d[3]; // soft bits, message, status
  if (!call.carve(SCRATCH_RX, {(size_t)cfg->llr_length, (size_t)cfg->message_length, sizeof(uint32_t)}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], llr, cfg->llr_length, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d[1], message, cfg->message_length, hipMemcpyHostToDevice)); // bytes the decoder leaves keep the caller's
  // The plan is made and released inside the call: the polar code is built (a second time after validate()), its tables are
  // allocated and uploaded with a blocking copy.  That is the price of the convenience form; a caller with more than a few
  // messages makes one plan over all of them.
  const uint64_t            zero = 0;
  nrphy_uci_decoder_plan_t* plan = nullptr;
  int                       rc   = nrphy_uci_decoder_plan_create(ctx, 1, cfg, &zero, &zero, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_uci_decoder_run(plan, (const int8_t*)d[0], d[1], (uint32_t*)d[2], ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(message, d[1], cfg->message_length, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(status, d[2], sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_uci_decoder_plan_destroy(plan);
  return rc;
}
