// Host side of the PUCCH format 0 and 1 receivers (pucch_kernels.hip): validation -- what pucch_pdu_validator_impl::is_valid
// (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:385-473) and the assertions of the two detectors refuse --, the
// plan's per-PUCCH constants (the cyclic shift index of every symbol, pucch_helper.h:79-108; the hop geometry of
// dmrs_pucch_processor_format1_impl.cpp:106-136; the symbol epochs the CFO estimate divides by) and the sequence tables in the
// reference's float expressions (complex_exponential_table, pucch_orthogonal_sequence).
#include "chest_host.h"

#include <array>
#include <cmath>

namespace {

#include "pucch_tables.inc"

constexpr float TWOPI_F = 2.0f * (float)M_PI;

// std::polar(1.0F, phase), cos and sin evaluated in double and rounded once (as the kernels evaluate theirs).
float2 polar1(float phase)
{
  return make_float2((float)std::cos((double)phase), (float)std::sin((double)phase));
}

bool hops(const nrphy_pucch_cfg_t& c)
{
  return c.second_hop_prb != NRPHY_PUCCH_NO_HOP;
}

int validate(const nrphy_pucch_cfg_t* cp, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  if (cp == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_pucch_cfg_t& c = *cp;
  if (c.format > NRPHY_PUCCH_FORMAT_1 || c.numerology > 4 || c.slot_index >= (10U << c.numerology)) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The BWP inside the grid, the PRBs inside the BWP (both formats occupy a single PRB per hop).
  const uint32_t grid_prb = grid_nof_subc / NRPHY_NRE;
  if (c.bwp_size_rb > grid_prb || c.bwp_start_rb > grid_prb - c.bwp_size_rb || c.starting_prb >= c.bwp_size_rb ||
      (hops(c) && c.second_hop_prb >= c.bwp_size_rb)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.start_symbol_index >= NRPHY_NSYMB || c.nof_symbols > NRPHY_NSYMB - c.start_symbol_index) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.initial_cyclic_shift > 11 || c.n_id > 1023 || c.nof_harq_ack > 2) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.format == NRPHY_PUCCH_FORMAT_0) {
    if (c.nof_symbols < 1 || c.nof_symbols > 2 || c.sr_opportunity > 1 || (c.nof_harq_ack == 0 && c.sr_opportunity == 0) ||
        c.time_domain_occ != 0) {
      return NRPHY_ERR_ARGUMENT;
    }
  } else {
    if (c.start_symbol_index > 10 || c.nof_symbols < 4 || c.sr_opportunity != 0 || c.time_domain_occ > 6) {
      return NRPHY_ERR_ARGUMENT;
    }
    // The shortest sequence the OCC index selects from: the data symbols of the first hop.
    if (c.time_domain_occ >= (hops(c) ? c.nof_symbols / 4 : c.nof_symbols / 2)) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  if (c.nof_rx_ports < 1 || c.nof_rx_ports > NRPHY_MAX_PORTS) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t i = 0; i != c.nof_rx_ports; ++i) {
    if (c.rx_ports[i] >= grid_nof_ports) {
      return NRPHY_ERR_ARGUMENT;
    }
    for (uint32_t j = 0; j != i; ++j) {
      if (c.rx_ports[j] == c.rx_ports[i]) {
        return NRPHY_ERR_ARGUMENT;
      }
    }
  }
  return NRPHY_OK;
}

// n_cs of the 14 symbols of slot n_slot: byte 14 n_slot + l of the Gold sequence c (TS 38.211 Section 5.2.1) with c_init = n_id,
// c(8 k + m) weighing 2^m (the reference reverses the byte it reads most significant bit first).
void cyclic_shift_hops(uint32_t n_id, uint32_t n_slot, uint8_t (&n_cs)[NRPHY_NSYMB])
{
  uint32_t x1 = 1, x2 = n_id; // bits n .. n + 30 of the two m-sequences
  const uint32_t first = 1600 + 8 * NRPHY_NSYMB * n_slot, last = first + 8 * NRPHY_NSYMB;
  std::memset(n_cs, 0, sizeof(n_cs));
  for (uint32_t n = 0; n != last; ++n) {
    if (n >= first && ((x1 ^ x2) & 1U)) {
      n_cs[(n - first) / 8] |= (uint8_t)(1U << ((n - first) % 8));
    }
    x1 = (x1 >> 1) | (((x1 ^ (x1 >> 3)) & 1U) << 30);
    x2 = (x2 >> 1) | (((x2 ^ (x2 >> 1) ^ (x2 >> 2) ^ (x2 >> 3)) & 1U) << 30);
  }
}

void build_tables(PucchTables& t)
{
  float2 e8[8];
  for (uint32_t k = 0; k != 8; ++k) {
    e8[k] = polar1((float)(2 * M_PI) * (float)k / 8.0f);
  }
  for (uint32_t u = 0; u != 30; ++u) {
    for (uint32_t n = 0; n != NRPHY_NRE; ++n) {
      t.base[u][n] = e8[(uint32_t)(8 + PUCCH_PHI_12[u][n]) % 8U];
    }
  }
  for (uint32_t k = 0; k != 24; ++k) {
    t.shift[k] = polar1((float)(2 * M_PI) * (float)k / 24.0f);
  }
  for (uint32_t n = 0; n != 7; ++n) {
    for (uint32_t i = 0; i != 7; ++i) {
      for (uint32_t m = 0; m != 7; ++m) {
        t.occ[n][i][m] = polar1(TWOPI_F * (float)PUCCH_OCC_PHI[n][i][m] / (float)(n + 1));
      }
    }
  }
}

} // namespace

struct nrphy_pucch_plan {
  nrphy_ctx*   ctx = nullptr;
  uint32_t     n = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  bool         has_ce = false;
  void*        d_arena  = nullptr;
  PucchDesc*   d_desc   = nullptr;
  PucchTables* d_tables = nullptr;
};

extern "C" int nrphy_pucch_validate(const nrphy_pucch_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_pucch_plan_destroy(nrphy_pucch_plan_t* plan)
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

extern "C" int nrphy_pucch_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pucch_cfg_t* cfgs, const uint32_t* grid_index,
                                       uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                       const uint64_t* ce_offset, nrphy_pucch_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  // A (port, symbol) row of a PRB is read as three 16-byte words: rows must start at a multiple of 16 bytes.
  if (ctx == nullptr || n == 0 || cfgs == nullptr || grid_index == nullptr || grid_nof_subc % 4 != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<PucchDesc>                          desc(n);
  std::map<uint32_t, std::array<uint8_t, NRPHY_NSYMB>> hop_cache; // (n_id, slot) -> n_cs: a cell's PUCCHs share them
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_pucch_cfg_t& c = cfgs[i];
    if (validate(&c, grid_nof_ports, grid_nof_subc) != NRPHY_OK || grid_index[i] >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    PucchDesc& d = desc[i];
    std::memset(&d, 0, sizeof(d));
    d.format         = c.format;
    d.grid_index     = grid_index[i];
    d.nof_rx_ports   = c.nof_rx_ports;
    d.first_symbol   = c.start_symbol_index;
    d.nof_symbols    = c.nof_symbols;
    d.prb[0]         = c.starting_prb + c.bwp_start_rb;
    d.prb[1]         = hops(c) ? c.second_hop_prb + c.bwp_start_rb : d.prb[0];
    d.hopping        = hops(c) ? 1U : 0U;
    d.u              = c.n_id % 30U;
    d.occ            = c.time_domain_occ;
    d.nof_harq_ack   = c.nof_harq_ack;
    d.sr_opportunity = c.sr_opportunity;
    d.scs_khz        = 15U << c.numerology;
    for (uint32_t k = 0; k != c.nof_rx_ports; ++k) {
      d.rx_ports[k] = (uint8_t)c.rx_ports[k];
    }
    const uint32_t key = (c.n_id << 8) | c.slot_index;
    auto           it  = hop_cache.find(key);
    if (it == hop_cache.end()) {
      uint8_t n_cs[NRPHY_NSYMB];
      cyclic_shift_hops(c.n_id, c.slot_index, n_cs);
      std::array<uint8_t, NRPHY_NSYMB> a;
      std::copy(n_cs, n_cs + NRPHY_NSYMB, a.begin());
      it = hop_cache.emplace(key, a).first;
    }
    for (uint32_t l = 0; l != c.nof_symbols; ++l) {
      d.alpha[l] = (uint8_t)((c.initial_cyclic_shift + it->second[c.start_symbol_index + l]) % NRPHY_NRE);
    }
    if (c.format == NRPHY_PUCCH_FORMAT_1) {
      float epoch[NRPHY_NSYMB];
      chest_symbol_epochs(c.numerology, epoch);
      // The first DM-RS symbol of each hop (an even symbol of the allocation) and the next DM-RS symbol of the slot.
      const uint32_t half = d.hopping ? c.nof_symbols / 2 : 0;
      const uint32_t s1   = c.start_symbol_index + ((half + 1U) & ~1U);
      d.cfo_dt[0]         = epoch[c.start_symbol_index + 2] - epoch[c.start_symbol_index];
      d.cfo_dt[1]         = s1 + 2 < NRPHY_NSYMB ? epoch[s1 + 2] - epoch[s1] : 0.f;
    }
    d.ce_offset = ce_offset != nullptr ? ce_offset[i] : 0;
  }
  std::vector<PucchTables> tables(1);
  build_tables(tables[0]);
  auto* plan           = new nrphy_pucch_plan;
  plan->ctx            = ctx;
  plan->n              = n;
  plan->grid_nof_ports = grid_nof_ports;
  plan->grid_nof_subc  = grid_nof_subc;
  plan->has_ce         = ce_offset != nullptr;
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PucchDesc));
  arena.add(&plan->d_tables, tables.data(), sizeof(PucchTables));
  void* unused = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_pucch_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pucch_run(nrphy_pucch_plan_t* plan, const void* d_grid, nrphy_pucch_result_t* d_result,
                               nrphy_pusch_chest_meas_t* d_meas, void* d_ch_est, void* stream)
{
  if (plan == nullptr || d_grid == nullptr || d_result == nullptr || (d_ch_est != nullptr && !plan->has_ce) ||
      ((uintptr_t)d_grid & 15U) != 0 || (((uintptr_t)d_result | (uintptr_t)d_meas | (uintptr_t)d_ch_est) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  PucchLaunch p;
  p.desc           = plan->d_desc;
  p.tables         = plan->d_tables;
  p.grid           = (const uint32_t*)d_grid;
  p.result         = d_result;
  p.meas           = d_meas;
  p.ch             = (uint32_t*)d_ch_est;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.n              = plan->n;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pucch(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_pucch_host(nrphy_ctx_t* ctx, const nrphy_pucch_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                                uint32_t grid_nof_subc, nrphy_pucch_result_t* result, nrphy_pusch_chest_meas_t* meas, void* ch_est)
{
  if (ctx == nullptr || grid == nullptr || result == nullptr || validate(cfg, grid_nof_ports, grid_nof_subc) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t ce_bytes   = (size_t)cfg->nof_rx_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t meas_bytes = NRPHY_MAX_PORTS * sizeof(nrphy_pusch_chest_meas_t);
  HostCall call(ctx);
  uint8_t* d[4]; // grid, result, measurements, estimate
  if (!call.carve(SCRATCH_RX, {grid_bytes, sizeof(nrphy_pucch_result_t), meas_bytes, ce_bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], grid, grid_bytes, hipMemcpyHostToDevice));
  if (ch_est != nullptr) {
    HIP_TRY(hipMemcpy(d[3], ch_est, ce_bytes, hipMemcpyHostToDevice)); // the kernel writes the allocation's part only
  }
  const uint32_t      zero = 0;
  const uint64_t      ce0  = 0;
  nrphy_pucch_plan_t* plan = nullptr;
  int rc = nrphy_pucch_plan_create(ctx, 1, cfg, &zero, 1, grid_nof_ports, grid_nof_subc, ch_est != nullptr ? &ce0 : nullptr, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_pucch_run(plan, d[0], (nrphy_pucch_result_t*)d[1], (nrphy_pusch_chest_meas_t*)d[2], ch_est != nullptr ? d[3] : nullptr,
                       ctx->stream);
  nrphy_pusch_chest_meas_t m[NRPHY_MAX_PORTS];
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(result, d[1], sizeof(*result), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(m, d[2], meas_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                         (ch_est != nullptr && hipMemcpy(ch_est, d[3], ce_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pucch_plan_destroy(plan);
  if (rc == NRPHY_OK && meas != nullptr) {
    std::memcpy(meas, m, cfg->nof_rx_ports * sizeof(nrphy_pusch_chest_meas_t));
  }
  return rc;
}
