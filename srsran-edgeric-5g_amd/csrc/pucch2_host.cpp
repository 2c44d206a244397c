// Host side of the PUCCH format 2 receiver (pucch2_kernels.hip): validation -- what
// pucch_pdu_validator_impl::is_valid(format2_configuration) (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:475-526),
// assert_format2_config (:323-383) and the assertions of pucch_demodulator_impl::demodulate refuse --, and the plan's per-PUCCH
// constants: the DM-RS seed of every symbol (dmrs_pucch_processor_format2_impl.cpp:35-41, a 64-bit product), the scrambling
// seed, the taps, virtual pilots and symbol epochs of chest_host.h, and the UCI decoder plan over the batch's messages.
#include "chest_host.h"

namespace {

constexpr float MAX_CODE_RATE = 0.80F; // pucch_constants::MAX_CODE_RATE

uint32_t nof_llr(const nrphy_pf2_cfg_t& c)
{
  return 2 * PF2_DATA_PER_PRB * c.nof_prb * c.nof_symbols;
}

int validate(const nrphy_pf2_cfg_t* cp, uint32_t grid_nof_ports, uint32_t grid_nof_subc, bool with_grid)
{
  if (cp == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_pf2_cfg_t& c = *cp;
  if (c.numerology > 4 || c.slot_index >= (10U << c.numerology) || c.rnti > 65535U || c.n_id > 1023U || c.n_id_0 > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The BWP inside the grid, the PRBs inside the BWP.
  if (c.bwp_size_rb > NRPHY_MAX_RB || c.bwp_start_rb > NRPHY_MAX_RB - c.bwp_size_rb || c.nof_prb < 1 || c.nof_prb > PF2_MAX_PRB ||
      c.starting_prb > c.bwp_size_rb || c.nof_prb > c.bwp_size_rb - c.starting_prb) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.nof_symbols < 1 || c.nof_symbols > PF2_MAX_SYMBOLS || c.start_symbol_index >= NRPHY_NSYMB ||
      c.nof_symbols > NRPHY_NSYMB - c.start_symbol_index) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.nof_csi_part2 != 0 || c.nof_harq_ack > 1706 || c.nof_sr > 1706 || c.nof_csi_part1 > 1706) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t A = c.nof_harq_ack + c.nof_sr + c.nof_csi_part1, E = nof_llr(c);
  if (A < 3 || A > 1706) { // FORMAT2_MIN_UCI_NBITS, FORMAT2_MAX_UCI_NBITS
    return NRPHY_ERR_ARGUMENT;
  }
  // pucch_format2_code_rate: payload and CRC bits (get_uci_nof_crc_bits) over the channel bits, compared in float.
  const uint32_t nof_blocks = ((A >= 360 && E >= 1088) || A >= 1013) ? 2 : 1;
  const uint32_t crc_bits   = nof_blocks * (A < 12 ? 0U : (A < 20 ? 6U : 11U));
  if ((float)(A + crc_bits) / (float)E > MAX_CODE_RATE) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_uci_decoder_cfg_t uci = {A, E, NRPHY_MOD_QPSK, 0};
  if (nrphy_uci_decoder_validate(&uci) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.nof_rx_ports < 1 || c.nof_rx_ports > NRPHY_MAX_PORTS) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t i = 0; i != c.nof_rx_ports; ++i) {
    for (uint32_t j = 0; j != i; ++j) {
      if (c.rx_ports[j] == c.rx_ports[i]) {
        return NRPHY_ERR_ARGUMENT;
      }
    }
  }
  if (!with_grid) {
    return NRPHY_OK;
  }
  if (c.bwp_start_rb + c.bwp_size_rb > grid_nof_subc / NRPHY_NRE) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t i = 0; i != c.nof_rx_ports; ++i) {
    if (c.rx_ports[i] >= grid_nof_ports) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  return NRPHY_OK;
}

} // namespace

struct nrphy_pf2_plan {
  nrphy_ctx*                ctx = nullptr;
  uint32_t                  n = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  bool                      has_ce = false;
  float                     demod_range = 0.f, demod_scale = 0.f;
  void*                     d_arena = nullptr;
  Pf2Desc*                  d_desc  = nullptr;
  const float2*             twiddle = nullptr; // the context's e^{j 2 pi i / 4096}: not the plan's to free
  nrphy_uci_decoder_plan_t* uci     = nullptr;
};

extern "C" int nrphy_pf2_validate(const nrphy_pf2_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, grid_nof_ports, grid_nof_subc, true);
}

extern "C" int nrphy_pf2_sizes(const nrphy_pf2_cfg_t* cfg, uint32_t* nof_llr_out, uint32_t* nof_payload_bits)
{
  if (nof_llr_out == nullptr || nof_payload_bits == nullptr || validate(cfg, 0, 0, false) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  *nof_llr_out      = nof_llr(*cfg);
  *nof_payload_bits = cfg->nof_harq_ack + cfg->nof_sr + cfg->nof_csi_part1;
  return NRPHY_OK;
}

extern "C" int nrphy_pf2_plan_destroy(nrphy_pf2_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  (void)nrphy_uci_decoder_plan_destroy(plan->uci);
  if (plan->d_arena != nullptr) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena);
  }
  delete plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pf2_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pf2_cfg_t* cfgs, const uint32_t* grid_index,
                                     uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* llr_offset,
                                     const uint64_t* message_offset, const uint64_t* ce_offset, nrphy_pf2_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  // The rows of a PRB are read as three 16-byte words: rows must start at a multiple of 16 bytes.
  if (ctx == nullptr || n == 0 || cfgs == nullptr || grid_index == nullptr || llr_offset == nullptr || message_offset == nullptr ||
      grid_nof_subc % 4 != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Pf2Desc>                 desc(n);
  std::vector<nrphy_uci_decoder_cfg_t> uci(n);
  DemodLaunch                          dp;
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_pf2_cfg_t& c = cfgs[i];
    if (validate(&c, grid_nof_ports, grid_nof_subc, true) != NRPHY_OK || grid_index[i] >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    Pf2Desc& d = desc[i];
    std::memset(&d, 0, sizeof(d));
    d.grid_index   = grid_index[i];
    d.nof_rx_ports = c.nof_rx_ports;
    d.nprb         = c.nof_prb;
    d.prb0         = c.bwp_start_rb + c.starting_prb;
    d.first_symbol = c.start_symbol_index;
    d.nof_symbols  = c.nof_symbols;
    float epoch[NRPHY_NSYMB];
    chest_symbol_epochs(c.numerology, epoch);
    for (uint32_t l = 0; l != c.nof_symbols; ++l) {
      const uint64_t nid = c.n_id_0, symbol = c.start_symbol_index + l;
      d.c_init_dmrs[l]   = (uint32_t)(((NRPHY_NSYMB * (uint64_t)c.slot_index + symbol + 1) * (2 * nid + 1) * (1ULL << 17) + 2 * nid) %
                                    (1ULL << 31));
      d.epoch[l]         = epoch[symbol];
    }
    d.c_init_data = (c.rnti << 15) + c.n_id;
    d.dmrs_words  = (2 * PF2_PILOTS_PER_PRB * (d.prb0 + d.nprb) + 31) / 32;
    d.ntaps       = chest_filter_taps(d.nprb, 3, d.taps);
    d.nof_v       = chest_nof_virtual_pilots(d.nprb, PF2_PILOTS_PER_PRB, d.ntaps);
    d.scs_hz      = 15000U << c.numerology;
    d.ls_scale    = 1.0f / ((float)c.nof_symbols * 1.0f);
    if (!demod_params(NRPHY_MOD_QPSK, PF2_DATA_PER_PRB * c.nof_prb * c.nof_symbols, dp)) {
      return NRPHY_ERR_ARGUMENT;
    }
    d.nof_vector = dp.nof_vector;
    for (uint32_t k = 0; k != c.nof_rx_ports; ++k) {
      d.rx_ports[k] = c.rx_ports[k];
    }
    d.llr_offset = llr_offset[i];
    d.ce_offset  = ce_offset != nullptr ? ce_offset[i] : 0;
    uci[i]       = {c.nof_harq_ack + c.nof_sr + c.nof_csi_part1, nof_llr(c), NRPHY_MOD_QPSK, 0};
  }
  // The time-alignment search's twiddles are the first quadrant of the context's table, built on first use.
  static_assert(PF2_TW_WORDS == 4096 / 4, "the first quadrant");
  const float2* twiddle = hipSetDevice(ctx->device) == hipSuccess ? get_twiddle_table(ctx, 4096) : nullptr;
  if (twiddle == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  auto* plan           = new nrphy_pf2_plan;
  plan->ctx            = ctx;
  plan->twiddle        = twiddle;
  plan->n              = n;
  plan->grid_nof_ports = grid_nof_ports;
  plan->grid_nof_subc  = grid_nof_subc;
  plan->has_ce         = ce_offset != nullptr;
  plan->demod_range    = dp.range;
  plan->demod_scale    = dp.scale;
  const int rc = nrphy_uci_decoder_plan_create(ctx, n, uci.data(), llr_offset, message_offset, &plan->uci);
  if (rc != NRPHY_OK) {
    nrphy_pf2_plan_destroy(plan);
    return rc;
  }
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(Pf2Desc));
  void* unused = nullptr;
  if (arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_pf2_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pf2_run(nrphy_pf2_plan_t* plan, const void* d_grid, int8_t* d_llr, uint8_t* d_message, uint32_t* d_status,
                             nrphy_pf2_csi_t* d_csi, nrphy_pusch_chest_meas_t* d_meas, void* d_ch_est, void* stream)
{
  // d_message and d_status both null: the receiver launch alone (the caller decodes d_llr with a plan of its own).
  if (plan == nullptr || d_grid == nullptr || d_llr == nullptr || (d_message == nullptr) != (d_status == nullptr) || d_csi == nullptr ||
      (d_ch_est != nullptr && !plan->has_ce) || ((uintptr_t)d_grid & 15U) != 0 ||
      (((uintptr_t)d_status | (uintptr_t)d_csi | (uintptr_t)d_meas | (uintptr_t)d_ch_est) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  Pf2Launch p;
  p.desc           = plan->d_desc;
  p.twiddle        = plan->twiddle;
  p.gold           = plan->ctx->d_gold;
  p.x1_words       = plan->ctx->d_x1;
  p.grid           = (const uint32_t*)d_grid;
  p.llr            = d_llr;
  p.csi            = d_csi;
  p.meas           = d_meas;
  p.ch             = (uint32_t*)d_ch_est;
  p.demod_range    = plan->demod_range;
  p.demod_scale    = plan->demod_scale;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.n              = plan->n;
  hipStream_t s    = stream ? (hipStream_t)stream : plan->ctx->stream;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pf2(p, s));
  return d_message != nullptr ? nrphy_uci_decoder_run(plan->uci, d_llr, d_message, d_status, s) : NRPHY_OK;
}

extern "C" int nrphy_pf2_host(nrphy_ctx_t* ctx, const nrphy_pf2_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                              uint32_t grid_nof_subc, uint8_t* message, uint32_t* status, nrphy_pf2_csi_t* csi,
                              nrphy_pusch_chest_meas_t* meas, void* ch_est, int8_t* llr)
{
  if (ctx == nullptr || grid == nullptr || message == nullptr || status == nullptr || csi == nullptr ||
      validate(cfg, grid_nof_ports, grid_nof_subc, true) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t A = cfg->nof_harq_ack + cfg->nof_sr + cfg->nof_csi_part1, E = nof_llr(*cfg);
  const size_t   grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t   ce_bytes   = (size_t)cfg->nof_rx_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t   meas_bytes = NRPHY_MAX_PORTS * sizeof(nrphy_pusch_chest_meas_t);
  HostCall call(ctx);
  uint8_t* d[7]; // grid, soft bits, message, status, csi, measurements, estimate
  if (!call.carve(SCRATCH_RX, {grid_bytes, (size_t)E, (size_t)A, sizeof(uint32_t), sizeof(nrphy_pf2_csi_t), meas_bytes, ce_bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], grid, grid_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d[2], message, A, hipMemcpyHostToDevice)); // bytes the decoder leaves keep the caller's
  if (ch_est != nullptr) {
    HIP_TRY(hipMemcpy(d[6], ch_est, ce_bytes, hipMemcpyHostToDevice)); // the kernel writes the allocation's part only
  }
  const uint32_t    zero = 0;
  const uint64_t    off0 = 0;
  nrphy_pf2_plan_t* plan = nullptr;
  int rc = nrphy_pf2_plan_create(ctx, 1, cfg, &zero, 1, grid_nof_ports, grid_nof_subc, &off0, &off0, ch_est != nullptr ? &off0 : nullptr,
                                 &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_pf2_run(plan, d[0], (int8_t*)d[1], d[2], (uint32_t*)d[3], (nrphy_pf2_csi_t*)d[4], (nrphy_pusch_chest_meas_t*)d[5],
                     ch_est != nullptr ? d[6] : nullptr, ctx->stream);
  nrphy_pusch_chest_meas_t m[NRPHY_MAX_PORTS];
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(message, d[2], A, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(status, d[3], sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(csi, d[4], sizeof(*csi), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(m, d[5], meas_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                         (llr != nullptr && hipMemcpy(llr, d[1], E, hipMemcpyDeviceToHost) != hipSuccess) ||
                         (ch_est != nullptr && hipMemcpy(ch_est, d[6], ce_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pf2_plan_destroy(plan);
  if (rc == NRPHY_OK && meas != nullptr) {
    std::memcpy(meas, m, cfg->nof_rx_ports * sizeof(nrphy_pusch_chest_meas_t));
  }
  return rc;
}
