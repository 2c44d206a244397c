// Host side of the OFDM PRACH demodulator (prach_demod_kernels.hip): the tables, validation, and the plan's window and bin
// arithmetic -- what ofdm_prach_demodulator_impl::demodulate derives from its configuration before it touches a sample
// (R/lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:31-157), in integer units of kappa (64 T_c: every time the reference
// forms here is a whole number of them), with get_prach_preamble_long_info / _short_info and get_prach_window_duration
// (R/lib/ran/prach/prach_preamble_information.cpp) and prach_frequency_mapping_get (prach_frequency_mapping.cpp) as tables.
#include "nrphy_host_internal.h"

#include <cmath>

namespace {

struct prach_demod_preamble_row_t {
  uint8_t  format, mu, last;
  uint16_t seq_len;
  uint8_t  ra_scs, nof_symbols, duration;
  uint32_t cp_kappa, symbols_kappa;
};
struct prach_demod_window_row_t {
  uint8_t  format, mu, start_symbol, nof_td;
  uint32_t kappa;
};
struct prach_demod_mapping_row_t {
  uint8_t nof_rb_ra, k_bar;
};
#include "prach_demod_tables.inc"

constexpr uint64_t KAPPA_HZ    = 30720000; // units of kappa per second
constexpr uint32_t HALF_MS     = 15360;    // 0.5 ms in kappa
constexpr uint32_t MAX_TD      = 7;        // seven two-symbol occasions fill a slot

const prach_demod_preamble_row_t* preamble_row(uint32_t format, uint32_t mu, bool last)
{
  const bool longf = format <= NRPHY_PRACH_FORMAT_3;
  for (const prach_demod_preamble_row_t& r : PRACH_DEMOD_PREAMBLE) {
    if (r.format == format && (longf || (r.mu == mu && r.last == (last ? 1 : 0)))) {
      return &r;
    }
  }
  return nullptr;
}

uint32_t scs_hz(uint32_t ra_scs)
{
  return ra_scs == NRPHY_PRACH_SCS_1_25 ? 1250U : ra_scs == NRPHY_PRACH_SCS_5 ? 5000U : 15000U << ra_scs;
}

// What one configuration comes to: sizes, bins, and per time-domain occasion the first sample behind the cyclic prefix.
struct Derived {
  nrphy_prach_demod_sizes_t sizes;
  uint32_t                  spacing, first_bin; // bins between frequency-domain occasions; bin of element 0 of occasion 0
  uint32_t                  symbol_offset[MAX_TD];
};

// kappa -> samples; false where that is no whole number (phy_time_unit::is_sample_accurate).
bool to_samples(uint64_t kappa, uint64_t srate, uint32_t* samples)
{
  if ((kappa * srate) % KAPPA_HZ != 0) {
    return false;
  }
  *samples = (uint32_t)((kappa * srate) / KAPPA_HZ);
  return true;
}

bool derive(const nrphy_prach_demod_cfg_t* cp, Derived& d)
{
  if (cp == nullptr) {
    return false;
  }
  const nrphy_prach_demod_cfg_t& c = *cp;
  if (c.format >= NRPHY_PRACH_FORMAT_COUNT || c.pusch_numerology > 3 || c.nof_rx_ports < 1 || c.nof_rx_ports > NRPHY_MAX_PORTS ||
      c.nof_prb_ul_grid < 1 || c.nof_prb_ul_grid > 275 || c.nof_fd_occasions < 1 || c.nof_fd_occasions > 8 ||
      c.nof_td_occasions < 1 || c.nof_td_occasions > MAX_TD || c.start_symbol > 13 || c.rb_offset >= 275 || c.srate_hz == 0) {
    return false;
  }
  const bool                        longf = c.format <= NRPHY_PRACH_FORMAT_3;
  const uint32_t                    mu    = c.pusch_numerology;
  const prach_demod_preamble_row_t* info  = preamble_row(c.format, mu, false);
  if (info == nullptr || (longf ? c.nof_td_occasions != 1 : c.start_symbol + info->duration * c.nof_td_occasions > 14)) {
    return false;
  }
  const prach_demod_mapping_row_t& map = PRACH_DEMOD_MAPPING[info->ra_scs][mu];
  if (map.nof_rb_ra == 0) { // reserved
    return false;
  }
  const uint32_t ra_hz = scs_hz(info->ra_scs);
  if (c.srate_hz % ra_hz != 0 || !dft_size_supported(c.srate_hz / ra_hz)) {
    return false;
  }
  const uint32_t N = c.srate_hz / ra_hz, K = (15000U << mu) / ra_hz, grid = c.nof_prb_ul_grid * K * 12;
  const uint32_t L = info->seq_len;
  d.spacing        = K * 12 * map.nof_rb_ra;
  const uint32_t k_start = K * 12 * c.rb_offset + map.k_bar;
  if (N <= grid || k_start + (c.nof_fd_occasions - 1) * d.spacing + L >= grid) {
    return false;
  }
  d.first_bin            = (k_start + N - grid / 2) % N;
  d.sizes.dft_size       = N;
  d.sizes.sequence_length = L;
  d.sizes.nof_symbols    = info->nof_symbols;
  d.sizes.window_samples = 0;
  const uint64_t srate   = c.srate_hz;
  for (uint32_t td = 0; td != c.nof_td_occasions; ++td) {
    const prach_demod_preamble_row_t* occ = preamble_row(c.format, mu, td == c.nof_td_occasions - 1);
    uint32_t start = (2192U >> mu) * (c.start_symbol + occ->duration * td);
    start += start > 0 ? 16 : 0;
    start += start > HALF_MS ? 16 : 0;
    uint32_t       cp  = occ->cp_kappa;
    const uint32_t end = start + cp + occ->symbols_kappa;
    if (!longf) {
      cp += start == 0 ? 16 : 0; // the occasion overlaps time 0
      cp += start <= HALF_MS && end >= HALF_MS ? 16 : 0;
    }
    uint32_t s_start = 0, s_cp = 0, s_len = 0;
    if (!to_samples(start, srate, &s_start) || !to_samples(cp, srate, &s_cp) || !to_samples(cp + occ->symbols_kappa, srate, &s_len)) {
      return false;
    }
    d.symbol_offset[td]    = s_start + s_cp;
    d.sizes.window_samples = std::max(d.sizes.window_samples, s_start + s_len);
  }
  if (!longf) {
    uint32_t window = 0;
    for (const prach_demod_window_row_t& r : PRACH_DEMOD_WINDOW) {
      if (r.format == c.format && r.mu == mu && r.start_symbol == c.start_symbol && r.nof_td == c.nof_td_occasions) {
        window = r.kappa;
      }
    }
    uint32_t s_window = 0;
    if (window == 0 || !to_samples(window, srate, &s_window)) {
      return false;
    }
    d.sizes.window_samples = std::max(d.sizes.window_samples, s_window);
  }
  return true;
}

struct Group { // the jobs of one LDS transform size: one launch
  uint32_t      lds_size, first, count;
  const float2* tw_lds;
};

} // namespace

struct nrphy_prach_demod_plan {
  nrphy_ctx*            ctx     = nullptr;
  void*                 d_arena = nullptr;
  PrachDemodDesc*       d_desc  = nullptr;
  PrachDemodJob*        d_jobs  = nullptr;
  std::vector<Group>    groups;
};

extern "C" int nrphy_prach_demod_validate(const nrphy_prach_demod_cfg_t* cfg)
{
  Derived d;
  return derive(cfg, d) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

extern "C" int nrphy_prach_demod_sizes(const nrphy_prach_demod_cfg_t* cfg, nrphy_prach_demod_sizes_t* sizes)
{
  Derived d;
  if (sizes == nullptr || !derive(cfg, d)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *sizes = d.sizes;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_demod_plan_destroy(nrphy_prach_demod_plan_t* plan)
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

extern "C" int nrphy_prach_demod_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_prach_demod_cfg_t* cfgs,
                                             const uint64_t* in_offset, uint64_t in_port_stride, const uint64_t* out_offset,
                                             uint64_t port_stride, uint64_t fd_stride, uint64_t td_stride, uint64_t symbol_stride,
                                             nrphy_prach_demod_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || in_offset == nullptr || out_offset == nullptr || n > (1U << 20)) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Derived> derived(n);
  for (uint32_t i = 0; i != n; ++i) {
    if (!derive(&cfgs[i], derived[i])) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  if (hipSetDevice(ctx->device) != hipSuccess) {
    return NRPHY_ERR_DEVICE;
  }
  // Jobs sorted by the size of their LDS transform; within a size in item order.
  std::vector<PrachDemodDesc>                desc(n);
  std::map<uint32_t, std::vector<PrachDemodJob>> by_size;
  for (uint32_t i = 0; i != n; ++i) {
    const Derived&                 d = derived[i];
    const nrphy_prach_demod_cfg_t& c = cfgs[i];
    uint32_t                       n1 = 1, n2 = d.sizes.dft_size;
    dft_split(d.sizes.dft_size, &n1, &n2);
    PrachDemodDesc& e = desc[i];
    e.tw_total        = get_twiddle(ctx, d.sizes.dft_size);
    if (e.tw_total == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
    e.fd_stride     = fd_stride;
    e.n1            = n1;
    e.n_total       = d.sizes.dft_size;
    e.seq_len       = d.sizes.sequence_length;
    e.spacing       = d.spacing;
    e.span          = (c.nof_fd_occasions - 1) * d.spacing + d.sizes.sequence_length;
    e.first_bin     = d.first_bin;
    e.first_bin_lds = d.first_bin % n2;
    std::vector<PrachDemodJob>& jobs = by_size[n2];
    for (uint32_t p = 0; p != c.nof_rx_ports; ++p) {
      for (uint32_t td = 0; td != c.nof_td_occasions; ++td) {
        for (uint32_t s = 0; s != d.sizes.nof_symbols; ++s) {
          PrachDemodJob job;
          job.in_offset  = in_offset[i] + p * in_port_stride + d.symbol_offset[td] + (uint64_t)s * d.sizes.dft_size;
          job.out_offset = out_offset[i] + p * port_stride + td * td_stride + s * symbol_stride;
          job.desc       = i;
          job.reserved   = 0;
          jobs.push_back(job);
        }
      }
    }
  }
  auto*                      plan = new nrphy_prach_demod_plan;
  std::vector<PrachDemodJob> jobs;
  plan->ctx = ctx;
  for (auto& kv : by_size) {
    const float2* tw = get_twiddle(ctx, kv.first);
    if (tw == nullptr) {
      delete plan;
      return NRPHY_ERR_DEVICE;
    }
    plan->groups.push_back({kv.first, (uint32_t)jobs.size(), (uint32_t)kv.second.size(), tw});
    jobs.insert(jobs.end(), kv.second.begin(), kv.second.end());
  }
  DeviceArena arena;
  void*       unused = nullptr;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PrachDemodDesc));
  arena.add(&plan->d_jobs, jobs.data(), jobs.size() * sizeof(PrachDemodJob));
  if (arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_prach_demod_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_window_demod_run(nrphy_prach_demod_plan_t* plan, const void* d_iq, uint32_t iq_format, float iq_scale,
                                            void* d_symbols, void* stream)
{
  const bool ci16 = iq_format == NRPHY_IQ_CI16;
  if (plan == nullptr || d_iq == nullptr || d_symbols == nullptr || iq_format > NRPHY_IQ_CI16 ||
      ((uintptr_t)d_iq & (ci16 ? 3U : 7U)) != 0 || ((uintptr_t)d_symbols & 7U) != 0 ||
      (ci16 && !(iq_scale > 0.f && std::isfinite(iq_scale)))) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(plan->ctx->device));
  for (const Group& g : plan->groups) {
    PrachDemodLaunch p;
    p.desc    = plan->d_desc;
    p.jobs    = plan->d_jobs + g.first;
    p.tw_lds  = g.tw_lds;
    p.samples = d_iq;
    p.symbols = (float2*)d_symbols;
    p.n_jobs  = g.count;
    p.ci16    = ci16 ? 1U : 0U;
    p.iq_gain = ci16 ? 1.0f / iq_scale : 1.0f;
    HIP_TRY(launch_prach_demod(g.lds_size, p, stream ? (hipStream_t)stream : plan->ctx->stream));
  }
  return NRPHY_OK;
}

extern "C" int nrphy_prach_demod_run(nrphy_prach_demod_plan_t* plan, const void* d_samples, void* d_symbols, void* stream)
{
  return nrphy_prach_window_demod_run(plan, d_samples, NRPHY_IQ_CF32, 1.0f, d_symbols, stream);
}

extern "C" int nrphy_prach_demodulate_host(nrphy_ctx_t* ctx, const nrphy_prach_demod_cfg_t* cfg, const void* samples,
                                           uint64_t in_port_stride, void* symbols, uint64_t port_stride, uint64_t fd_stride,
                                           uint64_t td_stride, uint64_t symbol_stride)
{
  Derived d;
  if (ctx == nullptr || samples == nullptr || symbols == nullptr || !derive(cfg, d)) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The spans the run's reads and writes cover: the last port's window, the last symbol of the last occasions of the last port.
  const size_t in_bytes  = ((size_t)(cfg->nof_rx_ports - 1) * in_port_stride + d.sizes.window_samples) * sizeof(float2);
  const size_t out_bytes = ((size_t)(cfg->nof_rx_ports - 1) * port_stride + (size_t)(cfg->nof_fd_occasions - 1) * fd_stride +
                            (size_t)(cfg->nof_td_occasions - 1) * td_stride + (size_t)(d.sizes.nof_symbols - 1) * symbol_stride +
                            d.sizes.sequence_length) * sizeof(float2);
  HostCall call(ctx);
  uint8_t* dev[2]; // samples, symbols
  if (!call.carve(SCRATCH_RX, {in_bytes, out_bytes}, dev)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(dev[0], samples, in_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dev[1], symbols, out_bytes, hipMemcpyHostToDevice)); // what the run leaves alone goes back as it came
  const uint64_t            zero = 0;
  nrphy_prach_demod_plan_t* plan = nullptr;
  int rc = nrphy_prach_demod_plan_create(ctx, 1, cfg, &zero, in_port_stride, &zero, port_stride, fd_stride, td_stride, symbol_stride,
                                         &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_prach_demod_run(plan, dev[0], dev[1], ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(symbols, dev[1], out_bytes, hipMemcpyDeviceToHost) != hipSuccess)) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_prach_demod_plan_destroy(plan);
  return rc;
}
