// Host side of the SRS channel estimator (srs_kernels.hip): validation -- what srs_validator_generic_impl::is_valid
// (R/lib/phy/upper/signal_processors/srs/srs_validator_generic_impl.cpp) and the assertions of
// srs_estimator_generic_impl::estimate and get_srs_information refuse --, the mapping of get_srs_information
// (R/lib/ran/srs/srs_information.cpp:39-105) and the plan's per-SRS constants: everything that does not depend on the grid.
#include "low_papr_host.h"

#include <cmath>
#include <complex>

namespace {

#include "pucch_tables.inc"
#include "srs_tables.inc"

struct SrsInfo {
  uint32_t M, k0, n_cs, n_cs_max, u;
};

// get_srs_information(resource, port) of a configuration validate() accepts.
SrsInfo srs_info(const nrphy_srs_cfg_t& c, uint32_t port)
{
  const uint32_t comb = c.comb_size;
  SrsInfo        s;
  s.M        = SRS_BANDWIDTH[c.configuration_index][c.bandwidth_index][0] * NRPHY_NRE / comb;
  s.u        = c.sequence_id % 30;
  s.n_cs_max = comb == 4 ? 12 : 8;
  s.n_cs     = (c.cyclic_shift + (s.n_cs_max * port) / c.nof_antenna_ports) % s.n_cs_max;
  uint32_t k_tc = c.comb_offset;
  if (c.cyclic_shift >= s.n_cs_max / 2 && c.cyclic_shift < s.n_cs_max && c.nof_antenna_ports == 4 && (port == 1 || port == 3)) {
    k_tc = (k_tc + comb / 2) % comb;
  }
  uint32_t sum = 0;
  for (uint32_t b = 0; b <= c.bandwidth_index; ++b) {
    const uint32_t m_srs = SRS_BANDWIDTH[c.configuration_index][b][0], N = SRS_BANDWIDTH[c.configuration_index][b][1];
    const uint32_t M_b   = m_srs * NRPHY_NRE / comb;
    sum += comb * M_b * (((4 * c.freq_position) / m_srs) % N);
  }
  s.k0 = c.freq_shift * NRPHY_NRE + k_tc + sum;
  return s;
}

int validate(const nrphy_srs_cfg_t* cp, uint32_t grid_nof_ports, uint32_t grid_nof_subc, bool with_grid)
{
  if (cp == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_srs_cfg_t& c = *cp;
  auto one_two_four = [](uint32_t v) { return v == 1 || v == 2 || v == 4; };
  if (c.numerology > 4 || !one_two_four(c.nof_antenna_ports) || !one_two_four(c.nof_symbols) || c.start_symbol >= NRPHY_NSYMB ||
      c.nof_symbols > NRPHY_NSYMB - c.start_symbol) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (c.configuration_index > 63 || c.sequence_id > 1023 || c.bandwidth_index > 3 || (c.comb_size != 2 && c.comb_size != 4) ||
      c.freq_position > 67 || c.freq_shift > 268 || c.freq_hopping > 3) {
    return NRPHY_ERR_ARGUMENT;
  }
  // srs_resource_configuration::is_valid, has_frequency_hopping, and the hopping the generator does not support.
  if (c.comb_offset >= c.comb_size || c.cyclic_shift > (c.comb_size == 2 ? 7U : 11U) || c.freq_hopping < c.bandwidth_index ||
      c.hopping != 0) {
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
  for (uint32_t i = 0; i != c.nof_rx_ports; ++i) {
    if (c.rx_ports[i] >= grid_nof_ports) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  for (uint32_t p = 0; p != c.nof_antenna_ports; ++p) {
    const SrsInfo s = srs_info(c, p);
    if (s.k0 + c.comb_size * (s.M - 1) >= grid_nof_subc) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  return NRPHY_OK;
}

// complex_exponential_table(size, 1): polar(1, float(2 pi) float(n) / float(size)).
std::vector<float2> unit_circle(uint32_t size)
{
  std::vector<float2> t(size);
  for (uint32_t n = 0; n != size; ++n) {
    const std::complex<float> v = std::polar(1.0F, static_cast<float>(2 * M_PI) * static_cast<float>(n) / static_cast<float>(size));
    t[n]                        = make_float2(v.real(), v.imag());
  }
  return t;
}

// The descriptor of a configuration validate() accepts (for the sequence alone: without a grid).
SrsDesc make_desc(const nrphy_srs_cfg_t& c, uint32_t grid_index)
{
  SrsDesc d;
  std::memset(&d, 0, sizeof(d));
  const SrsInfo  s0      = srs_info(c, 0);
  const uint32_t scs_khz = 15U << c.numerology;
  d.grid_index   = grid_index;
  d.nof_rx_ports = c.nof_rx_ports;
  d.nof_tx_ports = c.nof_antenna_ports;
  d.first_symbol = c.start_symbol;
  d.nof_symbols  = c.nof_symbols;
  d.comb         = c.comb_size;
  d.M            = s0.M;
  // Maximum measurable delay due to the cyclic shift, and time_alignment_estimator_dft_impl's max_ta_samples, both in double.
  const double max_ta = 1.0 / static_cast<double>(s0.n_cs_max * scs_khz * 1000 * c.comb_size);
  d.window       = static_cast<unsigned>(std::floor(max_ta * static_cast<double>(scs_khz * 1000 * SRS_DFT_SIZE)));
  d.scs_hz       = scs_khz * 1000;
  d.symbol_scale = (float)(1.0 / static_cast<float>(c.nof_symbols));
  if (s0.M >= 36) {
    d.n_zc = low_papr_prime_below(s0.M);
    d.q    = low_papr_zc_root(s0.u, d.n_zc);
  } else {
    for (uint32_t n = 0; n != s0.M; ++n) {
      d.phi[n] = s0.M == 12 ? PUCCH_PHI_12[s0.u][n] : SRS_PHI_24[s0.u][n];
    }
  }
  for (uint32_t i = 0; i != c.nof_rx_ports; ++i) {
    d.rx_ports[i] = c.rx_ports[i];
  }
  for (uint32_t p = 0; p != c.nof_antenna_ports; ++p) {
    const SrsInfo s = srs_info(c, p);
    d.k0[p]         = s.k0;
    d.cs_step[p]    = s.n_cs * SRS_CS_SIZE / s.n_cs_max;
  }
  return d;
}

} // namespace

struct nrphy_srs_plan {
  nrphy_ctx*    ctx = nullptr;
  uint32_t      n = 0, grid_nof_ports = 0, grid_nof_subc = 0;
  void*         d_arena = nullptr;
  SrsDesc*      d_desc  = nullptr;
  float2*       d_cs    = nullptr;
  float2*       d_cexp  = nullptr;
  const float2* d_tw    = nullptr; // the context's
};

extern "C" int nrphy_srs_validate(const nrphy_srs_cfg_t* cfg, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return validate(cfg, grid_nof_ports, grid_nof_subc, true);
}

extern "C" int nrphy_srs_info(const nrphy_srs_cfg_t* cfg, uint32_t antenna_port, uint32_t* sequence_length, uint32_t* initial_subcarrier,
                              uint32_t* n_cs, uint32_t* n_cs_max, uint32_t* u)
{
  if (sequence_length == nullptr || initial_subcarrier == nullptr || n_cs == nullptr || n_cs_max == nullptr || u == nullptr ||
      validate(cfg, 0, 0, false) != NRPHY_OK || antenna_port >= cfg->nof_antenna_ports) {
    return NRPHY_ERR_ARGUMENT;
  }
  const SrsInfo s     = srs_info(*cfg, antenna_port);
  *sequence_length    = s.M;
  *initial_subcarrier = s.k0;
  *n_cs               = s.n_cs;
  *n_cs_max           = s.n_cs_max;
  *u                  = s.u;
  return NRPHY_OK;
}

extern "C" int nrphy_srs_plan_destroy(nrphy_srs_plan_t* plan)
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

extern "C" int nrphy_srs_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_srs_cfg_t* cfgs, const uint32_t* grid_index,
                                     uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_srs_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || n > 65535 || cfgs == nullptr || grid_index == nullptr) { // an SRS is a row of the launch grid
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<SrsDesc> desc(n);
  for (uint32_t i = 0; i != n; ++i) {
    if (validate(&cfgs[i], grid_nof_ports, grid_nof_subc, true) != NRPHY_OK || grid_index[i] >= nof_grids) {
      return NRPHY_ERR_ARGUMENT;
    }
    desc[i] = make_desc(cfgs[i], grid_index[i]);
  }
  const std::vector<float2> cs = unit_circle(SRS_CS_SIZE), cexp = unit_circle(SRS_CEXP_SIZE);
  if (hipSetDevice(ctx->device) != hipSuccess) {
    return NRPHY_ERR_DEVICE;
  }
  auto* plan           = new nrphy_srs_plan;
  plan->ctx            = ctx;
  plan->n              = n;
  plan->grid_nof_ports = grid_nof_ports;
  plan->grid_nof_subc  = grid_nof_subc;
  plan->d_tw           = get_twiddle(ctx, SRS_DFT_SIZE);
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(SrsDesc));
  arena.add(&plan->d_cs, cs.data(), cs.size() * sizeof(float2));
  arena.add(&plan->d_cexp, cexp.data(), cexp.size() * sizeof(float2));
  void* unused = nullptr;
  if (plan->d_tw == nullptr || arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_srs_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_srs_run(nrphy_srs_plan_t* plan, const void* d_grid, nrphy_srs_result_t* d_result, void* stream)
{
  if (plan == nullptr || d_grid == nullptr || d_result == nullptr || ((uintptr_t)d_grid & 3U) != 0 || ((uintptr_t)d_result & 7U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  SrsLaunch p;
  p.desc           = plan->d_desc;
  p.twiddle        = plan->d_tw;
  p.cs_table       = plan->d_cs;
  p.cexp_table     = plan->d_cexp;
  p.grid           = (const uint32_t*)d_grid;
  p.result         = d_result;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.n              = plan->n;
  hipStream_t s    = stream ? (hipStream_t)stream : plan->ctx->stream;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_srs(p, s));
  return NRPHY_OK;
}

extern "C" int nrphy_srs_host(nrphy_ctx_t* ctx, const nrphy_srs_cfg_t* cfg, const void* grid, uint32_t grid_nof_ports,
                              uint32_t grid_nof_subc, nrphy_srs_result_t* result)
{
  if (ctx == nullptr || grid == nullptr || result == nullptr || validate(cfg, grid_nof_ports, grid_nof_subc, true) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  HostCall     call(ctx);
  uint8_t*     d[2]; // grid, result
  if (!call.carve(SCRATCH_RX, {grid_bytes, sizeof(nrphy_srs_result_t)}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], grid, grid_bytes, hipMemcpyHostToDevice));
  const uint32_t    zero = 0;
  nrphy_srs_plan_t* plan = nullptr;
  int               rc   = nrphy_srs_plan_create(ctx, 1, cfg, &zero, 1, grid_nof_ports, grid_nof_subc, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_srs_run(plan, d[0], (nrphy_srs_result_t*)d[1], ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(result, d[1], sizeof(*result), hipMemcpyDeviceToHost) != hipSuccess)) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_srs_plan_destroy(plan);
  return rc;
}

extern "C" int nrphy_srs_sequence_host(nrphy_ctx_t* ctx, const nrphy_srs_cfg_t* cfg, uint32_t antenna_port, float* out)
{
  if (ctx == nullptr || out == nullptr || validate(cfg, 0, 0, false) != NRPHY_OK || antenna_port >= cfg->nof_antenna_ports) {
    return NRPHY_ERR_ARGUMENT;
  }
  const SrsDesc             desc = make_desc(*cfg, 0);
  const std::vector<float2> cs   = unit_circle(SRS_CS_SIZE);
  const size_t              out_bytes = (size_t)desc.M * sizeof(float2);
  HostCall call(ctx);
  uint8_t* d[3]; // descriptor, cyclic shifts, sequence
  if (!call.carve(SCRATCH_RX, {sizeof(SrsDesc), cs.size() * sizeof(float2), out_bytes}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], &desc, sizeof(desc), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d[1], cs.data(), cs.size() * sizeof(float2), hipMemcpyHostToDevice));
  HIP_TRY(launch_srs_sequence((const SrsDesc*)d[0], (const float2*)d[1], antenna_port, desc.M, (float2*)d[2], ctx->stream));
  if (call.sync() != hipSuccess || hipMemcpy(out, d[2], out_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    return NRPHY_ERR_DEVICE;
  }
  return NRPHY_OK;
}
