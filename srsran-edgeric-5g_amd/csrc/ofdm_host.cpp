// Host side of ofdm_kernels.hip: the OFDM plan with its modulator, demodulator and timing entry points, and the stand-alone DFT.
#include "nrphy_host_internal.h"
#include "nrphy_trace.h"

#include <cmath>
#include <complex>
#include <map>
#include <mutex>
#include <new>
#include <vector>

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

namespace {

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

namespace {

int ofdm_demod(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_iq, const OfdmDemodRange& range,
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
  HIP_TRY(launch_ofdm_demod(p, nof_grids, d_iq, range, slot_index, window_offset, (uint32_t*)d_grid,
                            stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ofdm_demod_run(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const float* d_iq,
                                    const uint32_t* slot_index, uint32_t window_offset, void* d_grid, void* stream)
{
  if (plan == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  return ofdm_demod(plan, nof_grids, d_iq, OfdmDemodRange{0, plan->nsymb, false, 1.0f}, slot_index, window_offset, d_grid, stream);
}

// puxch_processor_impl::process_symbol (R/lib/phy/lower/processors/uplink/puxch/puxch_processor_impl.cpp:30-81) demodulates the
// ports of one symbol as soon as its samples are in: a run of symbols of every (grid, port), the other rows left alone.
extern "C" int nrphy_ofdm_demod_symbols(nrphy_ofdm_plan_t* plan, uint32_t nof_grids, const void* d_iq, uint32_t iq_format,
                                        float iq_scale, const uint32_t* d_slot_index, uint32_t first_symbol, uint32_t nof_symbols,
                                        uint32_t window_offset, void* d_grid, void* stream)
{
  if (plan == nullptr || nof_symbols == 0 || first_symbol >= plan->nsymb || nof_symbols > plan->nsymb - first_symbol ||
      iq_format > NRPHY_IQ_CI16 || (iq_format == NRPHY_IQ_CI16 && !(iq_scale > 0.f && std::isfinite(iq_scale)))) {
    return NRPHY_ERR_ARGUMENT;
  }
  const bool  ci16 = iq_format == NRPHY_IQ_CI16;
  const float gain = ci16 ? 1.0f / iq_scale : 1.0f; // srsvec::convert: const float gain = 1.0f / scale
  return ofdm_demod(plan, nof_grids, d_iq, OfdmDemodRange{first_symbol, nof_symbols, ci16, gain}, d_slot_index, window_offset, d_grid,
                    stream);
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
