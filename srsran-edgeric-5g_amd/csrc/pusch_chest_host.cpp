// Host side of the PUSCH DM-RS channel estimator (pusch_chest_kernels.hip): validation, and the plan's per-PUSCH constants --
// what dmrs_pusch_estimator_impl and port_channel_estimator_average_impl compute before touching the grid: c_init per DM-RS
// symbol (dmrs_pusch_estimator_impl.cpp:136-149), and the symbol start epochs and raised-cosine taps of chest_host.h.  For a
// transform-precoded PUSCH, in place of c_init, the constants of its low-PAPR DM-RS (low_papr_host.h and the phi tables).  One
// implementation: the calls without a low-PAPR description are the _ex calls with none.
#include "chest_host.h"
#include "low_papr_host.h"
#include "pusch_alloc_host.h"

#include <cmath>

namespace {

#include "pucch_tables.inc"
#include "pusch_lowpapr_tables.inc"
#include "srs_tables.inc"

bool low_papr(const nrphy_pusch_chest_lowpapr_t* lp)
{
  return lp != nullptr && lp->enabled != 0;
}

// The constants of r_{u,0}, u = n_rs_id mod 30, of length 6 nprb (group and sequence hopping off).
void fill_low_papr(PuschChestDesc& d, uint32_t n_rs_id, uint32_t nprb)
{
  const uint32_t u = n_rs_id % 30;
  d.lp.u           = u;
  if (nprb < 5) {
    d.lp.circle = 8;
    for (uint32_t n = 0; n != 6 * nprb; ++n) {
      d.lp.phi[n] = nprb == 1 ? PUSCH_PHI_6[u][n] : nprb == 2 ? PUCCH_PHI_12[u][n] : nprb == 3 ? PUSCH_PHI_18[u][n] : SRS_PHI_24[u][n];
    }
  } else if (nprb == 5) {
    d.lp.circle = 62;
  } else {
    d.lp.n_zc   = low_papr_prime_below(6 * nprb);
    d.lp.q      = low_papr_zc_root(u, d.lp.n_zc);
    d.lp.circle = 2 * d.lp.n_zc;
  }
}

int validate(const nrphy_pusch_chest_cfg_t* c, const nrphy_pusch_chest_lowpapr_t* lp, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  if (c == nullptr || c->dmrs_type != 1 || c->nof_tx_layers < 1 || c->nof_tx_layers > NRPHY_PUSCH_CHEST_MAX_LAYERS ||
      c->numerology > 4 || c->slot_index >= (10U << c->numerology) || c->scrambling_id > 65535U || c->n_scid > 1 ||
      !std::isfinite(c->scaling) || !(c->scaling > 0.f)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const PuschAllocation a = pusch_allocation(*c);
  if (!allocation_fits_grid(a, grid_nof_ports, grid_nof_subc) || nof_prb(a) == 0 || c->nof_symbols == 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The reference sizes its pilot buffer from the whole mask and reads only the symbols of [start, start + nof).
  const uint32_t inside = ((1U << c->nof_symbols) - 1U) << c->start_symbol_index;
  if ((c->dmrs_symbol_mask & inside) == 0 || (c->dmrs_symbol_mask & ~inside) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c->dc_position != NRPHY_PUSCH_CHEST_NO_DC && c->dc_position >= grid_nof_subc) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (lp != nullptr && (lp->enabled > 1 || (lp->enabled == 1 && (c->nof_tx_layers != 1 || c->n_scid != 0 || lp->n_rs_id > 1007U ||
                                                                 !nrphy_transform_precoding_nof_prb_valid(nof_prb(a)))))) {
    return NRPHY_ERR_ARGUMENT;
  }
  return NRPHY_OK;
}

} // namespace

struct nrphy_pusch_chest_plan {
  nrphy_ctx*      ctx = nullptr;
  uint32_t        n = 0, n_jobs = 0, n_gold = 0; // the jobs of the Gold PUSCHs come first
  uint32_t        nof_grids = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  void*           d_arena = nullptr;
  PuschChestDesc* d_desc  = nullptr;
  uint32_t*       d_jobs  = nullptr;
  uint16_t*       d_prbs  = nullptr;
  const float2*   twiddle = nullptr; // the context's e^{j 2 pi i / 2048}: not the plan's to free
  uint32_t*       d_rows  = nullptr;
  float2*         d_rot   = nullptr;
};

extern "C" int nrphy_pusch_chest_validate(const nrphy_pusch_chest_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, nullptr, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_pusch_chest_validate_ex(const nrphy_pusch_chest_cfg_t* cfg, const nrphy_pusch_chest_lowpapr_t* lp,
                                             uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, lp, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_pusch_chest_plan_destroy(nrphy_pusch_chest_plan_t* plan)
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

extern "C" int nrphy_pusch_chest_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_chest_cfg_t* cfgs,
                                             const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                             uint32_t grid_nof_subc, const uint64_t* ce_offset, nrphy_pusch_chest_plan_t** out)
{
  return nrphy_pusch_chest_plan_create_ex(ctx, n, cfgs, nullptr, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, ce_offset, out);
}

extern "C" int nrphy_pusch_chest_plan_create_ex(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_chest_cfg_t* cfgs,
                                                const nrphy_pusch_chest_lowpapr_t* lps, const uint32_t* grid_index, uint32_t nof_grids,
                                                uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* ce_offset,
                                                nrphy_pusch_chest_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || grid_index == nullptr || ce_offset == nullptr || n > 65535U) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<PuschChestDesc> desc(n);
  std::vector<uint32_t>       jobs, lp_jobs;
  std::vector<uint16_t>       prbs;
  uint64_t                    row_words = 0;
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_pusch_chest_cfg_t&     c  = cfgs[i];
    const nrphy_pusch_chest_lowpapr_t* lp = lps != nullptr ? &lps[i] : nullptr;
    if (validate(&c, lp, grid_nof_ports, grid_nof_subc) != NRPHY_OK || grid_index[i] >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    PuschChestDesc& d = desc[i];
    std::memset(&d, 0, sizeof(d));
    d.grid_index   = grid_index[i];
    d.nof_rx_ports = c.nof_rx_ports;
    d.nof_layers   = c.nof_tx_layers;
    d.prb_first    = (uint32_t)prbs.size();
    d.nprb         = append_prbs(pusch_allocation(c), grid_nof_subc, prbs);
    d.nwords       = (NRPHY_NRE * ((uint32_t)prbs.back() + 1) + 31) / 32;
    d.first_symbol = c.start_symbol_index;
    d.nof_symbols  = c.nof_symbols;
    for (uint32_t l = 0; l != NRPHY_NSYMB; ++l) {
      if ((c.dmrs_symbol_mask >> l) & 1U) {
        const uint64_t nid = c.scrambling_id;
        d.dmrs_symbol[d.nof_dmrs] = l;
        if (!low_papr(lp)) {
          d.c_init[d.nof_dmrs] = (uint32_t)(((NRPHY_NSYMB * (uint64_t)c.slot_index + l + 1) * (2 * nid + 1) * (1ULL << 17) +
                                             2 * nid + c.n_scid) %
                                            (1ULL << 31));
        }
        ++d.nof_dmrs;
      }
    }
    if (low_papr(lp)) {
      fill_low_papr(d, lp->n_rs_id, d.nprb);
    }
    chest_symbol_epochs(c.numerology, d.epoch);
    d.ntaps = chest_filter_taps(d.nprb, 2, d.taps);
    d.nof_v = chest_nof_virtual_pilots(d.nprb, 6, d.ntaps);
    d.dc    = c.dc_position;
    d.scs_hz = 15000U << c.numerology;
    for (uint32_t k = 0; k != c.nof_rx_ports; ++k) {
      d.rx_ports[k] = c.rx_ports[k];
    }
    d.beta       = c.scaling;
    d.ls_scale   = 1.0f / ((float)d.nof_dmrs * c.scaling);
    d.ce_offset  = ce_offset[i];
    d.row_offset = row_words;
    row_words += (uint64_t)c.nof_rx_ports * c.nof_tx_layers * NRPHY_NRE * d.nprb;
    for (uint32_t p = 0; p != c.nof_rx_ports; ++p) {
      for (uint32_t l = 0; l != c.nof_tx_layers; ++l) {
        (low_papr(lp) ? lp_jobs : jobs).push_back((i << 8) | (p << 4) | l);
      }
    }
  }
  const uint32_t n_gold = (uint32_t)jobs.size();
  jobs.insert(jobs.end(), lp_jobs.begin(), lp_jobs.end());
  // The time-alignment search's twiddles are the context's table, built on first use.
  const float2* twiddle = hipSetDevice(ctx->device) == hipSuccess ? get_twiddle_table(ctx, 2048) : nullptr;
  if (twiddle == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  auto* plan           = new nrphy_pusch_chest_plan;
  plan->ctx            = ctx;
  plan->twiddle        = twiddle;
  plan->n              = n;
  plan->n_jobs         = (uint32_t)jobs.size();
  plan->n_gold         = n_gold;
  plan->nof_grids      = nof_grids;
  plan->grid_nof_ports = grid_nof_ports;
  plan->grid_nof_subc  = grid_nof_subc;
  // One allocation, one upload of the host-built tables; behind them what the kernels write: the rows, then the rotations.
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PuschChestDesc));
  arena.add(&plan->d_jobs, jobs.data(), jobs.size() * sizeof(uint32_t));
  arena.add(&plan->d_prbs, prbs.data(), prbs.size() * sizeof(uint16_t));
  const size_t rows_bytes = (row_words * sizeof(uint32_t) + 255) & ~(size_t)255;
  if (arena.commit(&plan->d_arena, rows_bytes + jobs.size() * NRPHY_NSYMB * sizeof(float2), (void**)&plan->d_rows) != hipSuccess) {
    nrphy_pusch_chest_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  plan->d_rot = (float2*)((uint8_t*)plan->d_rows + rows_bytes);
  *out        = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_chest_run(nrphy_pusch_chest_plan_t* plan, const void* d_grid, void* d_ch_est, float* d_noise_vars,
                                     nrphy_pusch_chest_meas_t* d_meas, void* stream)
{
  if (plan == nullptr || d_grid == nullptr || d_ch_est == nullptr || d_noise_vars == nullptr ||
      (((uintptr_t)d_grid | (uintptr_t)d_ch_est | (uintptr_t)d_noise_vars | (uintptr_t)d_meas) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  PuschChestLaunch p;
  p.desc           = plan->d_desc;
  p.jobs           = plan->d_jobs;
  p.prbs           = plan->d_prbs;
  p.twiddle        = plan->twiddle;
  p.gold           = plan->ctx->d_gold;
  p.x1_words       = plan->ctx->d_x1;
  p.grid           = (const uint32_t*)d_grid;
  p.ch             = (uint32_t*)d_ch_est;
  p.noise_vars     = d_noise_vars;
  p.meas           = d_meas;
  p.rows           = plan->d_rows;
  p.rot            = plan->d_rot;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.n_jobs         = plan->n_jobs;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pusch_chest(p, plan->n_gold, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_chest_host(nrphy_ctx_t* ctx, const nrphy_pusch_chest_cfg_t* cfg, const void* grid,
                                      uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* ch_est, float* noise_vars,
                                      nrphy_pusch_chest_meas_t* meas)
{
  return nrphy_pusch_chest_host_ex(ctx, cfg, nullptr, grid, grid_nof_ports, grid_nof_subc, ch_est, noise_vars, meas);
}

extern "C" int nrphy_pusch_lowpapr_sequence_host(nrphy_ctx_t* ctx, uint32_t n_rs_id, uint32_t nof_prb, float* out)
{
  if (ctx == nullptr || out == nullptr || n_rs_id > 1007U || !nrphy_transform_precoding_nof_prb_valid(nof_prb)) {
    return NRPHY_ERR_ARGUMENT;
  }
  PuschChestDesc desc;
  std::memset(&desc, 0, sizeof(desc));
  desc.nprb = nof_prb;
  fill_low_papr(desc, n_rs_id, nof_prb);
  const size_t out_bytes = (size_t)6 * nof_prb * sizeof(float2);
  HostCall     call(ctx);
  uint8_t*     d[2]; // descriptor, sequence
  if (!call.carve(SCRATCH_RX, {sizeof(desc), out_bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], &desc, sizeof(desc), hipMemcpyHostToDevice));
  HIP_TRY(launch_pusch_lowpapr_sequence((const PuschChestDesc*)d[0], (float2*)d[1], ctx->stream));
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(out, d[1], out_bytes, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_chest_host_ex(nrphy_ctx_t* ctx, const nrphy_pusch_chest_cfg_t* cfg, const nrphy_pusch_chest_lowpapr_t* lp,
                                         const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, void* ch_est,
                                         float* noise_vars, nrphy_pusch_chest_meas_t* meas)
{
  if (ctx == nullptr || grid == nullptr || ch_est == nullptr || noise_vars == nullptr ||
      validate(cfg, lp, grid_nof_ports, grid_nof_subc) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t ce_bytes   = (size_t)cfg->nof_tx_layers * cfg->nof_rx_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t meas_bytes = NRPHY_MAX_PORTS * NRPHY_PUSCH_CHEST_MAX_LAYERS * sizeof(nrphy_pusch_chest_meas_t);
  HostCall call(ctx);
  uint8_t* d[4]; // grid, estimates, noise variances, measurements
  if (!call.carve(SCRATCH_RX, {grid_bytes, ce_bytes, NRPHY_MAX_PORTS * sizeof(float), meas_bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], grid, grid_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d[1], ch_est, ce_bytes, hipMemcpyHostToDevice)); // the kernels write the allocation's part only
  const uint32_t            zero = 0;
  const uint64_t            ce0  = 0;
  nrphy_pusch_chest_plan_t* plan = nullptr;
  int rc = nrphy_pusch_chest_plan_create_ex(ctx, 1, cfg, lp, &zero, 1, grid_nof_ports, grid_nof_subc, &ce0, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_pusch_chest_run(plan, d[0], d[1], (float*)d[2], (nrphy_pusch_chest_meas_t*)d[3], ctx->stream);
  std::vector<nrphy_pusch_chest_meas_t> m(NRPHY_MAX_PORTS * NRPHY_PUSCH_CHEST_MAX_LAYERS);
  float                                 nv[NRPHY_MAX_PORTS];
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(ch_est, d[1], ce_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(nv, d[2], sizeof(nv), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(m.data(), d[3], meas_bytes, hipMemcpyDeviceToHost) != hipSuccess)) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pusch_chest_plan_destroy(plan);
  if (rc == NRPHY_OK) {
    for (uint32_t i = 0; i != cfg->nof_rx_ports; ++i) {
      noise_vars[i] = nv[i];
    }
    if (meas != nullptr) {
      std::memcpy(meas, m.data(), cfg->nof_rx_ports * NRPHY_PUSCH_CHEST_MAX_LAYERS * sizeof(nrphy_pusch_chest_meas_t));
    }
  }
  return rc;
}
