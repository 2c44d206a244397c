// Host side of the PRACH detector (prach_kernels.hip): the threshold table, validation, and the plan's per-occasion constants --
// the integer arithmetic of prach_detector_generic_impl::detect before it touches the buffer (prach_detector_generic_impl.cpp:
// 97-172), in the reference's order of operations, with get_prach_preamble_long_info / _short_info
// (R/lib/ran/prach/prach_preamble_information.cpp), prach_cyclic_shifts_get (prach_cyclic_shifts.cpp, unrestricted columns) and
// the sequence numbers and closed-form constants of prach_generator_impl (prach_generator_impl.cpp:40-287).
#include "nrphy_host_internal.h"

#include <cmath>

namespace {

struct prach_threshold_row_t {
  uint8_t ports, scs, format, zcz;
  float   threshold;
  uint8_t margin, flag;
};
#include "prach_tables.inc"

constexpr double T_C = 1.0 / (480000.0 * 4096.0); // phy_time_unit::T_C

bool is_long(uint32_t format)
{
  return format <= NRPHY_PRACH_FORMAT_3;
}

// phy_time_unit::from_seconds(seconds).to_seconds()
double round_to_tc(double seconds)
{
  const double  tc_units_dbl = seconds / T_C;
  const int64_t tc_units     = (int64_t)(tc_units_dbl * 10.0);
  return (double)(tc_units / 10 + (tc_units % 10) / 5) * T_C;
}

uint32_t scs_hz(uint32_t ra_scs)
{
  return ra_scs == NRPHY_PRACH_SCS_1_25 ? 1250U : ra_scs == NRPHY_PRACH_SCS_5 ? 5000U : 15000U << ra_scs;
}

// Symbols per occasion and cyclic prefix in units of kappa (the mixed formats as a non-last occasion, as the detector asks).
void preamble_info(uint32_t format, uint32_t ra_scs, uint32_t* nof_symbols, uint32_t* cp_kappa)
{
  static const uint16_t SYMBOLS[NRPHY_PRACH_FORMAT_COUNT] = {1, 2, 4, 4, 2, 4, 6, 2, 12, 1, 4, 2, 4, 6};
  static const uint16_t CP[NRPHY_PRACH_FORMAT_COUNT] = {3168, 21024, 4688, 3168, 288, 576, 864, 216, 936, 1240, 2048, 288, 576, 864};
  *nof_symbols = SYMBOLS[format];
  *cp_kappa    = is_long(format) ? CP[format] : (uint32_t)CP[format] >> ra_scs;
}

const prach_threshold_row_t* find_row(const nrphy_prach_cfg_t& c)
{
  for (const prach_threshold_row_t& r : PRACH_THRESHOLDS) {
    if (r.ports == c.nof_rx_ports && r.scs == c.ra_scs && r.format == c.format && r.zcz == c.zero_correlation_zone) {
      return &r;
    }
  }
  return nullptr;
}

// Everything detect() derives from the configuration; false where the configuration is refused.
bool derive(const nrphy_prach_cfg_t* cp, PrachDesc& d)
{
  if (cp == nullptr) {
    return false;
  }
  const nrphy_prach_cfg_t& c = *cp;
  if (c.restricted_set != 0 || c.format >= NRPHY_PRACH_FORMAT_COUNT || c.ra_scs >= NRPHY_PRACH_SCS_COUNT ||
      c.zero_correlation_zone > 15 || c.nof_preamble_indices == 0 || c.start_preamble_index > NRPHY_PRACH_MAX_PREAMBLES ||
      c.nof_preamble_indices > NRPHY_PRACH_MAX_PREAMBLES - c.start_preamble_index || c.nof_rx_ports < 1 ||
      c.nof_rx_ports > NRPHY_MAX_PORTS) {
    return false;
  }
  const bool longf = is_long(c.format);
  if (longf ? c.ra_scs != (c.format == NRPHY_PRACH_FORMAT_3 ? NRPHY_PRACH_SCS_5 : NRPHY_PRACH_SCS_1_25) : c.ra_scs > NRPHY_PRACH_SCS_120) {
    return false;
  }
  const uint32_t L = longf ? PRACH_L_LONG : PRACH_L_SHORT, N = longf ? PRACH_N_LONG : PRACH_N_SHORT;
  if (c.root_sequence_index >= L - 1) {
    return false;
  }
  std::memset(&d, 0, sizeof(d));
  if ((c.threshold != 0.f) != (c.win_margin != 0)) {
    return false;
  }
  if (c.win_margin != 0) {
    if (!std::isfinite(c.threshold) || !(c.threshold > 0.f)) {
      return false;
    }
    d.threshold  = c.threshold;
    d.win_margin = c.win_margin;
  } else {
    const prach_threshold_row_t* row = find_row(c);
    if (row == nullptr || row->flag == 0) {
      return false;
    }
    d.threshold  = row->threshold;
    d.win_margin = row->margin;
  }
  uint32_t cp_kappa = 0;
  preamble_info(c.format, c.ra_scs, &d.nof_symbols, &cp_kappa);
  d.is_long      = longf;
  d.nof_rx_ports = c.nof_rx_ports;
  d.n_cs = (c.ra_scs == NRPHY_PRACH_SCS_1_25 ? PRACH_NCS_1_25 : c.ra_scs == NRPHY_PRACH_SCS_5 ? PRACH_NCS_5 : PRACH_NCS_SHORT)[c.zero_correlation_zone];
  d.nof_shifts    = 1;
  d.nof_sequences = 64;
  if (d.n_cs != 0) {
    d.nof_shifts    = std::min<uint32_t>(NRPHY_PRACH_MAX_PREAMBLES, L / d.n_cs);
    d.nof_sequences = (64 + d.nof_shifts - 1) / d.nof_shifts;
  }
  const uint32_t hz   = scs_hz(c.ra_scs);
  d.sample_rate_hz    = (double)(N * hz);
  const double   cp_duration = (double)((int64_t)cp_kappa * 64) * T_C;
  const uint32_t cp_prach    = (uint32_t)std::floor(cp_duration * L * hz);
  uint32_t       win         = d.n_cs == 0 ? cp_prach : std::min(d.n_cs, cp_prach);
  d.win_width                = (win * N) / L;
  uint32_t max_delay         = d.n_cs == 0 ? cp_prach : std::min(std::max(d.n_cs, 1U) - 1U, cp_prach);
  d.max_delay                = (max_delay * N) / L;
  d.delay_end                = (uint32_t)std::ceil((double)(float)d.max_delay * 0.8);
  d.start                    = c.start_preamble_index;
  d.end                      = c.start_preamble_index + c.nof_preamble_indices;
  // What the kernel's LDS arrays and its single wrap of the reference window assume (true of every table row).
  if (d.win_width == 0 || d.win_width > N || d.nof_shifts * d.win_width > N || 2 * d.win_margin + d.win_width > N ||
      d.win_margin > N) {
    return false;
  }
  for (uint32_t w = 0; w != d.nof_shifts; ++w) {
    if ((N - (d.n_cs * w * N) / L) % N + d.win_width > N) {
      return false;
    }
  }
  while ((1U << d.group_log2) < d.win_width && d.group_log2 < 6) {
    ++d.group_log2;
  }
  d.modsq_scale        = 1.0f / (float)(N * L * L);
  d.win_scale          = (float)N / (float)L;
  d.time_resolution_s  = (float)round_to_tc(1.0 / d.sample_rate_hz);
  d.time_advance_max_s = (float)round_to_tc((double)d.max_delay * 0.8 / d.sample_rate_hz);
  return true;
}

PrachSequence sequence(bool longf, uint32_t root_index, uint32_t shift)
{
  PrachSequence s;
  s.u      = longf ? PRACH_ROOT_LONG[root_index % (PRACH_L_LONG - 1)] : PRACH_ROOT_SHORT[root_index % (PRACH_L_SHORT - 1)];
  s.factor = longf ? PRACH_FACTOR_LONG[s.u] : PRACH_FACTOR_SHORT[s.u];
  s.offset = longf ? PRACH_OFFSET_LONG[s.u] : PRACH_OFFSET_SHORT[s.u];
  s.shift  = (uint16_t)shift;
  return s;
}

// The context's tables, built on first use: the generator's exponentials with the reference's float expression
// (complex_exponential_table: std::polar(amplitude, float(2 pi) * float(i) / float(size))), the twiddles in double rounded once.
const PrachTables* get_tables(nrphy_ctx* ctx)
{
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  if (ctx->d_prach != nullptr) {
    return ctx->d_prach;
  }
  std::vector<PrachTables> t(1);
  for (int k = 0; k != 2; ++k) {
    const uint32_t size      = 4 * (k == 0 ? PRACH_L_LONG : PRACH_L_SHORT);
    const float    amplitude = std::sqrt((float)(k == 0 ? PRACH_L_LONG : PRACH_L_SHORT));
    float2*        table     = k == 0 ? t[0].cexp_long : t[0].cexp_short;
    for (uint32_t i = 0; i != size; ++i) {
      const float phase = (float)(2.0 * M_PI) * (float)i / (float)size;
      table[i]          = make_float2(amplitude * std::cos(phase), amplitude * std::sin(phase));
    }
    const uint32_t n  = k == 0 ? PRACH_N_LONG : PRACH_N_SHORT;
    float2*        tw = k == 0 ? t[0].tw_long : t[0].tw_short;
    for (uint32_t i = 0; i != n; ++i) {
      const double a = 2.0 * M_PI * (double)i / (double)n;
      tw[i]          = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  }
  PrachTables* d = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || upload(&d, t.data(), sizeof(PrachTables)) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  ctx->d_prach = d;
  return d;
}

} // namespace

struct nrphy_prach_plan {
  nrphy_ctx*         ctx = nullptr;
  uint32_t           n = 0, n_jobs_long = 0, n_jobs_short = 0, metric_stride = 0;
  uint64_t           port_stride = 0, symbol_stride = 0;
  const PrachTables* d_tables = nullptr;
  void*              d_arena  = nullptr;
  PrachDesc*         d_desc   = nullptr;
  uint32_t*          d_jobs_long  = nullptr;
  uint32_t*          d_jobs_short = nullptr;
  uint32_t*          d_rssi_ok    = nullptr;
};

extern "C" int nrphy_prach_threshold(const nrphy_prach_cfg_t* cfg, float* threshold, uint32_t* win_margin, uint32_t* flag)
{
  const prach_threshold_row_t* row = cfg != nullptr ? find_row(*cfg) : nullptr;
  if (row == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (threshold != nullptr) {
    *threshold = row->threshold;
  }
  if (win_margin != nullptr) {
    *win_margin = row->margin;
  }
  if (flag != nullptr) {
    *flag = row->flag;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_prach_validate(const nrphy_prach_cfg_t* cfg)
{
  PrachDesc d;
  return derive(cfg, d) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

extern "C" uint32_t nrphy_prach_window_width(const nrphy_prach_cfg_t* cfg)
{
  PrachDesc d;
  return derive(cfg, d) ? d.win_width : 0;
}

extern "C" int nrphy_prach_plan_destroy(nrphy_prach_plan_t* plan)
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

extern "C" uint32_t nrphy_prach_plan_metric_stride(const nrphy_prach_plan_t* plan)
{
  return plan != nullptr ? plan->metric_stride : 0;
}

extern "C" int nrphy_prach_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_prach_cfg_t* cfgs, const uint64_t* sym_offset,
                                       uint64_t port_stride, uint64_t symbol_stride, nrphy_prach_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || sym_offset == nullptr || n > (1U << 24) - 1) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<PrachDesc> desc(n);
  std::vector<uint32_t>  jobs_long, jobs_short;
  uint32_t               stride = 0;
  for (uint32_t i = 0; i != n; ++i) {
    PrachDesc& d = desc[i];
    if (!derive(&cfgs[i], d)) {
      return NRPHY_ERR_ARGUMENT;
    }
    d.sym_offset = sym_offset[i];
    stride       = std::max(stride, d.win_width);
    for (uint32_t s = 0; s != d.nof_sequences; ++s) {
      d.seq[s] = sequence(d.is_long != 0, cfgs[i].root_sequence_index + s, 0);
      (d.is_long ? jobs_long : jobs_short).push_back((i << 8) | s);
    }
  }
  const PrachTables* tables = get_tables(ctx);
  if (tables == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  auto* plan          = new nrphy_prach_plan;
  plan->ctx           = ctx;
  plan->n             = n;
  plan->n_jobs_long   = (uint32_t)jobs_long.size();
  plan->n_jobs_short  = (uint32_t)jobs_short.size();
  plan->metric_stride = stride;
  plan->port_stride   = port_stride;
  plan->symbol_stride = symbol_stride;
  plan->d_tables      = tables;
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PrachDesc));
  arena.add(&plan->d_jobs_long, jobs_long.data(), jobs_long.size() * sizeof(uint32_t));
  arena.add(&plan->d_jobs_short, jobs_short.data(), jobs_short.size() * sizeof(uint32_t));
  if (hipSetDevice(ctx->device) != hipSuccess ||
      arena.commit(&plan->d_arena, n * sizeof(uint32_t), (void**)&plan->d_rssi_ok) != hipSuccess) {
    nrphy_prach_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_run(nrphy_prach_plan_t* plan, const void* d_symbols, nrphy_prach_result_t* d_result,
                               nrphy_prach_preamble_t* d_preambles, float* d_metric, void* stream)
{
  if (plan == nullptr || d_symbols == nullptr || d_result == nullptr || d_preambles == nullptr ||
      (((uintptr_t)d_symbols | (uintptr_t)d_result) & 7U) != 0 || (((uintptr_t)d_preambles | (uintptr_t)d_metric) & 3U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  PrachLaunch p;
  p.desc          = plan->d_desc;
  p.jobs_long     = plan->d_jobs_long;
  p.jobs_short    = plan->d_jobs_short;
  p.tables        = plan->d_tables;
  p.symbols       = (const float2*)d_symbols;
  p.result        = d_result;
  p.preambles     = d_preambles;
  p.metric        = d_metric;
  p.rssi_ok       = plan->d_rssi_ok;
  p.port_stride   = plan->port_stride;
  p.symbol_stride = plan->symbol_stride;
  p.n             = plan->n;
  p.n_jobs_long   = plan->n_jobs_long;
  p.n_jobs_short  = plan->n_jobs_short;
  p.metric_stride = plan->metric_stride;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_prach_detect(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_prach_detect_host(nrphy_ctx_t* ctx, const nrphy_prach_cfg_t* cfg, const void* symbols, uint64_t port_stride,
                                       uint64_t symbol_stride, nrphy_prach_result_t* result, nrphy_prach_preamble_t* preambles,
                                       float* metric)
{
  PrachDesc d;
  if (ctx == nullptr || symbols == nullptr || result == nullptr || preambles == nullptr || !derive(cfg, d)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t L = d.is_long ? PRACH_L_LONG : PRACH_L_SHORT;
  // The span the occasion's reads cover: the last symbol of the last port.
  const size_t sym_bytes    = ((size_t)(d.nof_rx_ports - 1) * port_stride + (size_t)(d.nof_symbols - 1) * symbol_stride + L) * sizeof(float2);
  const size_t pre_bytes    = NRPHY_PRACH_MAX_PREAMBLES * sizeof(nrphy_prach_preamble_t);
  const size_t metric_bytes = (size_t)NRPHY_PRACH_MAX_PREAMBLES * d.win_width * sizeof(float);
  HostCall call(ctx);
  uint8_t* dev[4]; // symbols, result, preambles, metric
  if (!call.carve(SCRATCH_RX, {sym_bytes, sizeof(nrphy_prach_result_t), pre_bytes, metric_bytes}, dev)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(dev[0], symbols, sym_bytes, hipMemcpyHostToDevice));
  const uint64_t      zero = 0;
  nrphy_prach_plan_t* plan = nullptr;
  int                 rc   = nrphy_prach_plan_create(ctx, 1, cfg, &zero, port_stride, symbol_stride, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_prach_run(plan, dev[0], (nrphy_prach_result_t*)dev[1], (nrphy_prach_preamble_t*)dev[2],
                       metric != nullptr ? (float*)dev[3] : nullptr, ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(result, dev[1], sizeof(nrphy_prach_result_t), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(preambles, dev[2], pre_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                         (metric != nullptr && hipMemcpy(metric, dev[3], metric_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_prach_plan_destroy(plan);
  return rc;
}

extern "C" int nrphy_prach_generate_host(nrphy_ctx_t* ctx, const nrphy_prach_cfg_t* cfg, uint32_t preamble_index, float* y)
{
  if (ctx == nullptr || cfg == nullptr || y == nullptr || cfg->restricted_set != 0 || cfg->format >= NRPHY_PRACH_FORMAT_COUNT ||
      cfg->zero_correlation_zone > 15 || preamble_index >= NRPHY_PRACH_MAX_PREAMBLES) {
    return NRPHY_ERR_ARGUMENT;
  }
  // prach_generator_impl::generate: the long formats take their own spacing's N_CS table, every short one the 15 kHz table.
  const bool     longf = is_long(cfg->format);
  const uint32_t L     = longf ? PRACH_L_LONG : PRACH_L_SHORT;
  if (cfg->root_sequence_index >= L - 1) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t n_cs = (!longf ? PRACH_NCS_SHORT : cfg->format == NRPHY_PRACH_FORMAT_3 ? PRACH_NCS_5 : PRACH_NCS_1_25)[cfg->zero_correlation_zone];
  uint32_t root = cfg->root_sequence_index + preamble_index, shift = 0;
  if (n_cs != 0) {
    const uint32_t per_root = L / n_cs;
    root                    = cfg->root_sequence_index + preamble_index / per_root;
    shift                   = (preamble_index % per_root) * n_cs;
  }
  const PrachTables* tables = get_tables(ctx);
  HostCall           call(ctx);
  float2*            d_y = call.mem<float2>(SCRATCH_RX, L * sizeof(float2));
  if (tables == nullptr || d_y == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(launch_prach_generate(tables, sequence(longf, root, shift), longf, d_y, ctx->stream));
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(y, d_y, L * sizeof(float2), hipMemcpyDeviceToHost));
  return NRPHY_OK;
}
