// Host side of the channel equaliser and the PUSCH demodulator (pusch_demod_kernels.hip): validation, codeword sizes, the plan's
// work list, and the host-span forms.  The plan does on the host what pusch_demodulator_impl::demodulate does before its loops
// (pusch_demodulator_impl.cpp:135-160: the RE masks of data and DM-RS symbols, c_init) and cuts every OFDM symbol's data RE into
// work items of up to PUSCH_DEMOD_THREADS, each with its codeword bit offset and its place in the symbol's demapper span.  A
// transform-precoded PUSCH (the _ex forms with NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING) gets one item per OFDM symbol, in a list
// of its own, and the stage list and twiddle table of its transform size.  For the EVM (nrphy_pusch_demod_run_evm) the plan also
// says where each OFDM symbol's items start and how many equalised symbols it has, and holds one more partial sum per item.
#include "pusch_alloc_host.h"

#include <cmath>

namespace {

// Data subcarriers of a PRB on a DM-RS symbol: those dmrs_type::get_dmrs_prb_mask(cdm) leaves (R/include/srsran/phy/upper/
// dmrs_mapping.h:76-91).  Type 1: CDM group 0 = even subcarriers, 1 = odd.  Type 2: group g = {2g, 2g+1, 2g+6, 2g+7}.
// Returns false for a combination the type does not allow.
bool dmrs_data_mask(uint32_t type, uint32_t cdm, uint32_t& mask)
{
  if (type == 1 && cdm >= 1 && cdm <= 2) {
    mask = cdm == 1 ? 0xAAAU : 0U;
    return true;
  }
  if (type == 2 && cdm >= 1 && cdm <= 3) {
    mask = 0xFFFU;
    for (uint32_t g = 0; g != cdm; ++g) {
      mask &= ~((3U << (2 * g)) | (3U << (2 * g + 6)));
    }
    return true;
  }
  return false;
}

uint32_t popcount12(uint32_t m)
{
  return (uint32_t)__builtin_popcount(m & 0xFFFU);
}

// Data RE of OFDM symbol l (0 outside the allocation's symbols).
uint32_t symbol_re(const nrphy_pusch_demod_cfg_t& c, uint32_t l, uint32_t nprb, uint32_t dmrs_mask)
{
  if (l < c.start_symbol_index || l >= c.start_symbol_index + c.nof_symbols) {
    return 0;
  }
  return nprb * (((c.dmrs_symbol_mask >> l) & 1U) ? popcount12(dmrs_mask) : NRPHY_NRE);
}

// NRPHY_MOD_* of a configuration's qm (pi/2-BPSK is the only modulation of one bit on PUSCH).
uint32_t modulation_of(uint32_t qm)
{
  return qm == 1 ? NRPHY_MOD_PI2_BPSK : qm;
}

// `features`: what the caller opted into beyond the first contract (NRPHY_PUSCH_DEMOD_*); 0 refuses both.
int validate(const nrphy_pusch_demod_cfg_t* c, uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint32_t features)
{
  uint32_t dmrs_mask = 0;
  if (c == nullptr || (features & ~(NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING | NRPHY_PUSCH_DEMOD_PI2_BPSK)) != 0 ||
      c->transform_precoding > ((features & NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING) ? 1U : 0U) ||
      !(c->qm == 2 || c->qm == 4 || c->qm == 6 || c->qm == 8 || (c->qm == 1 && (features & NRPHY_PUSCH_DEMOD_PI2_BPSK))) ||
      c->nof_tx_layers < 1 || c->nof_tx_layers > 2 || c->equalizer > NRPHY_EQ_MMSE ||
      (c->nof_tx_layers == 2 && (c->equalizer != NRPHY_EQ_ZF || (c->nof_rx_ports != 2 && c->nof_rx_ports != 4))) ||
      !dmrs_data_mask(c->dmrs_type, c->nof_cdm_groups_without_data, dmrs_mask)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const PuschAllocation a = pusch_allocation(*c);
  if (!allocation_fits_grid(a, grid_nof_ports, grid_nof_subc) || (c->dmrs_symbol_mask >> NRPHY_NSYMB) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t nprb = nof_prb(a);
  // Transform precoding: one layer (pusch_demodulator_impl.cpp:188-190); DM-RS type 1 with both CDM groups kept free of data
  // (TS 38.214 Section 6.2.2), so that every symbol with data carries 12 RE per PRB -- the reference would run a half-size
  // transform on a DM-RS symbol otherwise; a PRB count the deprecoder has.
  if (c->transform_precoding != 0 && (c->nof_tx_layers != 1 || c->dmrs_type != 1 || c->nof_cdm_groups_without_data != 2 ||
                                      !nrphy_transform_precoding_nof_prb_valid(nprb))) {
    return NRPHY_ERR_ARGUMENT;
  }
  uint32_t nre = 0;
  for (uint32_t l = 0; l != NRPHY_NSYMB; ++l) {
    nre += symbol_re(*c, l, nprb, dmrs_mask);
  }
  return nre == 0 ? NRPHY_ERR_ARGUMENT : NRPHY_OK;
}

} // namespace

struct nrphy_pusch_demod_plan {
  nrphy_ctx*            ctx = nullptr;
  uint32_t              n = 0, n_items = 0, n_tp_items = 0;
  uint32_t              nof_grids = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  std::vector<uint64_t> cw_bits;
  void*                 d_arena   = nullptr;
  PuschDemodDesc*       d_desc    = nullptr;
  PuschDemodItem*       d_items   = nullptr;
  PuschTpItem*          d_tp_items = nullptr;
  MixedDftPlan*         d_dft     = nullptr;
  uint16_t*             d_prbs    = nullptr;
  DemodLaunch*          d_demod   = nullptr;
  double*               d_partial = nullptr;
  PuschEvmDesc*         d_evm_desc = nullptr;
  double*               d_evm_partial = nullptr; // behind d_partial
};

extern "C" int nrphy_pusch_demod_validate(const nrphy_pusch_demod_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, grid_nof_ports, grid_nof_subc, 0);
}

extern "C" int nrphy_pusch_demod_validate_ex(const nrphy_pusch_demod_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                             uint32_t features)
{
  return validate(cfg, grid_nof_ports, grid_nof_subc, features);
}

extern "C" uint64_t nrphy_pusch_demod_codeword_bits(const nrphy_pusch_demod_cfg_t* cfg)
{
  uint32_t dmrs_mask = 0;
  if (cfg == nullptr || cfg->qm > 8 || cfg->nof_tx_layers > NRPHY_MAX_LAYERS ||
      !dmrs_data_mask(cfg->dmrs_type, cfg->nof_cdm_groups_without_data, dmrs_mask)) {
    return 0;
  }
  const uint32_t nprb = nof_prb(pusch_allocation(*cfg));
  uint64_t       nre  = 0;
  for (uint32_t l = 0; l != NRPHY_NSYMB; ++l) {
    nre += symbol_re(*cfg, l, nprb, dmrs_mask);
  }
  return nre * cfg->nof_tx_layers * cfg->qm;
}

extern "C" int nrphy_pusch_demod_plan_destroy(nrphy_pusch_demod_plan_t* plan)
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

extern "C" int nrphy_pusch_demod_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_demod_cfg_t* cfgs,
                                             const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                             uint32_t grid_nof_subc, const uint64_t* ce_offset, nrphy_pusch_demod_plan_t** out)
{
  return nrphy_pusch_demod_plan_create_ex(ctx, n, cfgs, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, ce_offset, 0, out);
}

extern "C" int nrphy_pusch_demod_plan_create_ex(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_demod_cfg_t* cfgs,
                                                const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                                uint32_t grid_nof_subc, const uint64_t* ce_offset, uint32_t features,
                                                nrphy_pusch_demod_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || grid_index == nullptr || ce_offset == nullptr || n > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<PuschDemodDesc> desc(n);
  std::vector<PuschEvmDesc>   evm_desc(n);
  std::vector<PuschDemodItem> items;
  std::vector<PuschTpItem>    tp_items; // transform-precoded PUSCHs: one item per OFDM symbol, a kernel of their own
  std::vector<MixedDftPlan>   dfts;     // one per distinct size
  std::vector<uint16_t>       prbs;
  std::vector<uint64_t>       cw_bits(n);
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_pusch_demod_cfg_t& c = cfgs[i];
    if (validate(&c, grid_nof_ports, grid_nof_subc, features) != NRPHY_OK || grid_index[i] >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    uint32_t dmrs_mask = 0;
    dmrs_data_mask(c.dmrs_type, c.nof_cdm_groups_without_data, dmrs_mask);
    PuschDemodDesc& d = desc[i];
    std::memset(&d, 0, sizeof(d));
    d.grid_index      = grid_index[i];
    d.nof_rx_ports    = c.nof_rx_ports;
    d.nof_layers      = c.nof_tx_layers;
    d.qm              = c.qm;
    d.equalizer       = c.equalizer;
    d.c_init          = c.rnti * (1U << 15) + c.n_id;
    d.prb_first       = (uint32_t)prbs.size();
    d.dmrs_re_per_prb = popcount12(dmrs_mask);
    for (uint32_t k = 0, j = 0; k != NRPHY_NRE; ++k) {
      if ((dmrs_mask >> k) & 1U) {
        d.dmrs_subc[j++] = (uint8_t)k;
      }
    }
    for (uint32_t k = 0; k != c.nof_rx_ports; ++k) {
      d.rx_ports[k] = c.rx_ports[k];
    }
    d.ce_offset = ce_offset[i];
    const uint32_t nprb = append_prbs(pusch_allocation(c), grid_nof_subc, prbs);
    const uint32_t nb   = c.nof_tx_layers * c.qm;
    uint32_t       bit  = 0;
    uint32_t       dft  = 0;
    if (c.transform_precoding != 0) {
      MixedDftPlan mp;
      mixed_dft_stages(nprb, mp); // validate() has checked the size
      for (; dft != dfts.size() && dfts[dft].n != mp.n; ++dft) {
      }
      if (dft == dfts.size()) {
        dfts.push_back(mp);
      }
    }
    d.item_first = (uint32_t)(c.transform_precoding != 0 ? tp_items.size() : items.size());
    PuschEvmDesc& e = evm_desc[i];
    std::memset(&e, 0, sizeof(e));
    for (uint32_t l = 0; l != NRPHY_NSYMB; ++l) {
      const uint32_t nre = symbol_re(c, l, nprb, dmrs_mask);
      if (nre == 0) {
        continue; // pusch_demodulator_impl.cpp:172-175
      }
      e.item_first[e.nof_symbols] = (uint32_t)(c.transform_precoding != 0 ? tp_items.size() : items.size());
      e.count[e.nof_symbols++]    = nre * c.nof_tx_layers;
      DemodLaunch dp;
      demod_params(modulation_of(c.qm), nre * c.nof_tx_layers, dp);
      if (c.transform_precoding != 0) {
        PuschTpItem it;
        it.pusch      = i;
        it.symbol     = l;
        it.count      = nre;
        it.bit_offset = bit;
        it.nof_vector = dp.nof_vector;
        it.dft        = dft;
        tp_items.push_back(it);
        bit += nre * nb;
        continue;
      }
      for (uint32_t first = 0; first < nre; first += PUSCH_DEMOD_THREADS) {
        PuschDemodItem it;
        it.pusch      = i;
        it.symbol     = l;
        it.dmrs       = (c.dmrs_symbol_mask >> l) & 1U;
        it.re_first   = first;
        it.count      = std::min(PUSCH_DEMOD_THREADS, nre - first);
        it.bit_offset = bit + first * nb;
        it.span_pos   = first * c.nof_tx_layers;
        it.nof_vector = dp.nof_vector;
        items.push_back(it);
      }
      bit += nre * nb;
    }
    d.nof_items = (uint32_t)(c.transform_precoding != 0 ? tp_items.size() : items.size()) - d.item_first;
    e.item_first[e.nof_symbols] = d.item_first + d.nof_items;
    cw_bits[i]  = bit;
  }
  // The partial sums of the transform-precoded items follow those of the plain ones.
  for (uint32_t i = 0; i != n; ++i) {
    if (cfgs[i].transform_precoding != 0) {
      desc[i].item_first += (uint32_t)items.size();
      for (uint32_t k = 0; k <= evm_desc[i].nof_symbols; ++k) {
        evm_desc[i].item_first[k] += (uint32_t)items.size();
      }
    }
  }
  DemodLaunch demod[5];
  for (uint32_t m = 0; m != 4; ++m) {
    demod_params(2 * (m + 1), 0, demod[m]);
  }
  demod_params(NRPHY_MOD_PI2_BPSK, 0, demod[4]);
  if (hipSetDevice(ctx->device) != hipSuccess) {
    return NRPHY_ERR_DEVICE;
  }
  for (MixedDftPlan& mp : dfts) {
    mp.twiddle = get_twiddle_table(ctx, mp.n);
    if (mp.twiddle == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  auto* plan           = new nrphy_pusch_demod_plan;
  plan->ctx            = ctx;
  plan->n              = n;
  plan->n_items        = (uint32_t)items.size();
  plan->n_tp_items     = (uint32_t)tp_items.size();
  plan->nof_grids      = nof_grids;
  plan->grid_nof_ports = grid_nof_ports;
  plan->grid_nof_subc  = grid_nof_subc;
  plan->cw_bits        = std::move(cw_bits);
  // One allocation, one upload of the host-built tables; behind them what the kernel writes: two partial sums per item, and a
  // third, in an array of its own behind those, where a run takes the EVM.
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PuschDemodDesc));
  arena.add(&plan->d_items, items.data(), items.size() * sizeof(PuschDemodItem));
  arena.add(&plan->d_prbs, prbs.data(), prbs.size() * sizeof(uint16_t));
  arena.add(&plan->d_demod, demod, sizeof(demod));
  arena.add(&plan->d_tp_items, tp_items.data(), tp_items.size() * sizeof(PuschTpItem));
  arena.add(&plan->d_dft, dfts.data(), dfts.size() * sizeof(MixedDftPlan));
  arena.add(&plan->d_evm_desc, evm_desc.data(), evm_desc.size() * sizeof(PuschEvmDesc));
  if (arena.commit(&plan->d_arena, (items.size() + tp_items.size()) * 3 * sizeof(double), (void**)&plan->d_partial) !=
      hipSuccess) {
    nrphy_pusch_demod_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  plan->d_evm_partial = plan->d_partial + 2 * (items.size() + tp_items.size());
  *out = plan;
  return NRPHY_OK;
}

extern "C" uint64_t nrphy_pusch_demod_plan_codeword_bits(const nrphy_pusch_demod_plan_t* plan, uint32_t i)
{
  return (plan == nullptr || i >= plan->n) ? 0 : plan->cw_bits[i];
}

extern "C" int nrphy_pusch_demod_run(nrphy_pusch_demod_plan_t* plan, const void* d_grid, const void* d_ch_est,
                                     const float* d_noise_vars, int8_t* d_llr, uint64_t llr_stride, float* d_sinr_db, void* stream)
{
  return nrphy_pusch_demod_run_evm(plan, d_grid, d_ch_est, d_noise_vars, d_llr, llr_stride, d_sinr_db, nullptr, stream);
}

extern "C" int nrphy_pusch_demod_run_evm(nrphy_pusch_demod_plan_t* plan, const void* d_grid, const void* d_ch_est,
                                         const float* d_noise_vars, int8_t* d_llr, uint64_t llr_stride, float* d_sinr_db,
                                         float* d_evm, void* stream)
{
  if (plan == nullptr || d_grid == nullptr || d_ch_est == nullptr || d_noise_vars == nullptr || d_llr == nullptr ||
      (((uintptr_t)d_grid | (uintptr_t)d_ch_est | (uintptr_t)d_noise_vars | (uintptr_t)d_sinr_db | (uintptr_t)d_evm) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (plan->n > 1) {
    for (uint64_t g : plan->cw_bits) {
      if (llr_stride < g) {
        return NRPHY_ERR_ARGUMENT;
      }
    }
  }
  PuschDemodLaunch p;
  p.desc           = plan->d_desc;
  p.items          = plan->d_items;
  p.tp_items       = plan->d_tp_items;
  p.dft            = plan->d_dft;
  p.n_tp_items     = plan->n_tp_items;
  p.prbs          = plan->d_prbs;
  p.demod          = plan->d_demod;
  p.gold           = plan->ctx->d_gold;
  p.x1_words       = plan->ctx->d_x1;
  p.grid           = (const uint32_t*)d_grid;
  p.ch             = (const uint32_t*)d_ch_est;
  p.noise          = d_noise_vars;
  p.llr            = d_llr;
  p.llr_stride     = llr_stride;
  p.partial        = plan->d_partial;
  p.sinr           = d_sinr_db;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.n_pusch        = plan->n;
  p.n_items        = plan->n_items;
  p.evm_desc       = plan->d_evm_desc;
  p.evm_partial    = plan->d_evm_partial;
  p.evm            = d_evm;
  // modulation_mapper_lut_impl.cpp:58-64: scaling = std::sqrt(1 / avg_power) in float, avg_power = 2, 10, 42, 170; the
  // pi/2-BPSK tables hold (float)M_SQRT1_2.
  const float avg_power[4] = {2.0f, 10.0f, 42.0f, 170.0f};
  for (uint32_t m = 0; m != 4; ++m) {
    p.evm_scale[m] = std::sqrt(1.0f / avg_power[m]);
  }
  p.evm_scale[4] = (float)M_SQRT1_2;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pusch_demod(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

namespace {

bool equalize_args_ok(uint32_t algorithm, uint32_t nof_layers, uint32_t nof_rx_ports, float tx_scaling)
{
  return algorithm <= NRPHY_EQ_MMSE && nof_rx_ports >= 1 && nof_rx_ports <= NRPHY_MAX_PORTS && tx_scaling > 0.f &&
         (nof_layers == 1 || (nof_layers == 2 && algorithm == NRPHY_EQ_ZF && (nof_rx_ports == 2 || nof_rx_ports == 4)));
}

} // namespace

extern "C" int nrphy_pusch_demodulate_host(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid,
                                           uint32_t grid_nof_ports, uint32_t grid_nof_subc, const void* ch_est,
                                           const float* noise_vars, int8_t* llr, float* sinr_db)
{
  return nrphy_pusch_demodulate_host_ex(ctx, cfg, grid, grid_nof_ports, grid_nof_subc, ch_est, noise_vars, 0, llr, sinr_db);
}

extern "C" int nrphy_pusch_demodulate_host_ex(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid,
                                              uint32_t grid_nof_ports, uint32_t grid_nof_subc, const void* ch_est,
                                              const float* noise_vars, uint32_t features, int8_t* llr, float* sinr_db)
{
  return nrphy_pusch_demodulate_host_evm(ctx, cfg, grid, grid_nof_ports, grid_nof_subc, ch_est, noise_vars, features, llr, sinr_db,
                                         nullptr);
}

extern "C" int nrphy_pusch_demodulate_host_evm(nrphy_ctx_t* ctx, const nrphy_pusch_demod_cfg_t* cfg, const void* grid,
                                               uint32_t grid_nof_ports, uint32_t grid_nof_subc, const void* ch_est,
                                               const float* noise_vars, uint32_t features, int8_t* llr, float* sinr_db, float* evm)
{
  if (ctx == nullptr || grid == nullptr || ch_est == nullptr || noise_vars == nullptr || llr == nullptr ||
      validate(cfg, grid_nof_ports, grid_nof_subc, features) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint64_t G          = nrphy_pusch_demod_codeword_bits(cfg);
  const size_t   grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t   ce_bytes   = (size_t)cfg->nof_tx_layers * cfg->nof_rx_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  float          nv[NRPHY_MAX_PORTS] = {};
  for (uint32_t i = 0; i != cfg->nof_rx_ports; ++i) {
    nv[i] = noise_vars[i];
  }
  HostCall call(ctx);
  uint8_t* d[6]; // grid, estimates, noise variances, soft bits, SINR, EVM
  if (!call.carve(SCRATCH_RX, {grid_bytes, ce_bytes, sizeof(nv), (size_t)G, sizeof(float), sizeof(float)}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  void *  d_grid = d[0], *d_ce = d[1];
  float*  d_nv   = (float*)d[2];
  int8_t* d_llr  = (int8_t*)d[3];
  float*  d_sinr = (float*)d[4];
  float*  d_evm  = evm != nullptr ? (float*)d[5] : nullptr; // without it the launches are those of nrphy_pusch_demod_run
  HIP_TRY(hipMemcpy(d_grid, grid, grid_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ce, ch_est, ce_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nv, nv, sizeof(nv), hipMemcpyHostToDevice));
  const uint32_t            zero = 0;
  const uint64_t            ce0  = 0;
  nrphy_pusch_demod_plan_t* plan = nullptr;
  int rc = nrphy_pusch_demod_plan_create_ex(ctx, 1, cfg, &zero, 1, grid_nof_ports, grid_nof_subc, &ce0, features, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_pusch_demod_run_evm(plan, d_grid, d_ce, d_nv, d_llr, G, d_sinr, d_evm, ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess ||
                         hipMemcpy(llr, d_llr, G, hipMemcpyDeviceToHost) != hipSuccess ||
                         (sinr_db != nullptr && hipMemcpy(sinr_db, d_sinr, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) ||
                         (evm != nullptr && hipMemcpy(evm, d_evm, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pusch_demod_plan_destroy(plan);
  return rc;
}

extern "C" int nrphy_channel_equalize(nrphy_ctx_t* ctx, uint32_t algorithm, uint32_t n_batch, uint32_t nof_re, uint32_t nof_layers,
                                      uint32_t nof_rx_ports, const void* d_rx, const void* d_ch, const float* d_noise_vars,
                                      float tx_scaling, float* d_eq, float* d_eq_nvars, void* stream)
{
  if (ctx == nullptr || !equalize_args_ok(algorithm, nof_layers, nof_rx_ports, tx_scaling) || n_batch > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (n_batch == 0 || nof_re == 0) {
    return NRPHY_OK;
  }
  if (d_rx == nullptr || d_ch == nullptr || d_noise_vars == nullptr || d_eq == nullptr || d_eq_nvars == nullptr ||
      (((uintptr_t)d_rx | (uintptr_t)d_ch | (uintptr_t)d_noise_vars | (uintptr_t)d_eq_nvars) & 3U) != 0 ||
      ((uintptr_t)d_eq & 7U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  EqualizeLaunch p;
  p.algorithm    = algorithm;
  p.n_batch      = n_batch;
  p.nof_re       = nof_re;
  p.nof_layers   = nof_layers;
  p.nof_rx_ports = nof_rx_ports;
  p.tx_scaling   = tx_scaling;
  p.rx           = (const uint32_t*)d_rx;
  p.ch           = (const uint32_t*)d_ch;
  p.noise        = d_noise_vars;
  p.eq           = d_eq;
  p.eq_nvars     = d_eq_nvars;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(launch_channel_equalize(p, stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_channel_equalize_host(nrphy_ctx_t* ctx, uint32_t algorithm, uint32_t nof_re, uint32_t nof_layers,
                                           uint32_t nof_rx_ports, const void* rx, const void* ch, const float* noise_vars,
                                           float tx_scaling, float* eq, float* eq_nvars)
{
  if (ctx == nullptr || !equalize_args_ok(algorithm, nof_layers, nof_rx_ports, tx_scaling)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (nof_re == 0) {
    return NRPHY_OK;
  }
  if (rx == nullptr || ch == nullptr || noise_vars == nullptr || eq == nullptr || eq_nvars == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t rx_bytes = (size_t)nof_rx_ports * nof_re * 4, ch_bytes = rx_bytes * nof_layers;
  const size_t out      = (size_t)nof_re * nof_layers;
  HostCall call(ctx);
  uint8_t* d[5]; // received RE, estimates, noise variances, equalised RE, their noise variances
  if (!call.carve(SCRATCH_RX, {rx_bytes, ch_bytes, nof_rx_ports * sizeof(float), out * 8, out * 4}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  void * d_rx = d[0], *d_ch = d[1];
  float *d_nv = (float*)d[2], *d_eq = (float*)d[3], *d_ev = (float*)d[4];
  HIP_TRY(hipMemcpy(d_rx, rx, rx_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ch, ch, ch_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nv, noise_vars, nof_rx_ports * sizeof(float), hipMemcpyHostToDevice));
  const int rc = nrphy_channel_equalize(ctx, algorithm, 1, nof_re, nof_layers, nof_rx_ports, d_rx, d_ch, d_nv, tx_scaling, d_eq,
                                        d_ev, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(eq, d_eq, out * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(eq_nvars, d_ev, out * 4, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}
