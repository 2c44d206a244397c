// Arithmetic of port_channel_estimator_average_impl (R/lib/phy/upper/signal_processors/port_channel_estimator_average_impl.cpp)
// shared by the kernels that run it with the `filter` smoothing strategy: the PUSCH DM-RS estimator (pusch_chest_kernels.hip) and
// the PUCCH format 2 receiver (pucch2_kernels.hip).  One copy, so that both round alike.  The operations it is made of --
// constants, products, the phasor, the time-alignment search's comparison -- are exact_device.h's, which the other receivers
// share too.  The raised-cosine table and the taps derived from it are plan-time constants: chest_host.h.
#pragma once

#include "bits_device.h"
#include "exact_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t CHEST_TA_BINS = 2 * PUSCH_CHEST_TA_WINDOW;

// compute_v_pilots: a linear fit of |.| and of the unwrapped argument of n pilots, evaluated at i + offset.  In two steps, so that
// a kernel may fit on one lane and evaluate on several: the fit (serial by nature: unwrap_list, R/lib/srsvec/unwrap.cpp, and four
// running sums), and the value at one position.
struct VirtualPilotFit {
  float slope_abs, icp_abs, slope_arg, icp_arg;
};

__device__ inline VirtualPilotFit virtual_pilot_fit(const float* abs_, float* arg, uint32_t n)
{
  float k = 0.f;
  for (uint32_t i = 0; i + 1 < n; ++i) {
    const float old_a = arg[i], next_a = arg[i + 1];
    arg[i]            = __fadd_rn(arg[i], __fmul_rn(__fmul_rn(2.0f, k), PI_F));
    const float jump  = __fsub_rn(next_a, old_a);
    if (fabsf(jump) > PI_F) {
      k = __fsub_rn(k, jump < 0.f ? -1.0f : 1.0f);
    }
  }
  arg[n - 1] = __fadd_rn(arg[n - 1], __fmul_rn(__fmul_rn(2.0f, k), PI_F));
  const float nf        = (float)n;
  const float mean_x    = __fdiv_rn(__fdiv_rn((float)(n * (n - 1)), 2.0f), nf);
  const float norm_x_sq = __fdiv_rn((float)((n - 1) * n * (2 * n - 1)), 6.0f);
  const float den       = __fsub_rn(norm_x_sq, __fmul_rn(__fmul_rn(nf, mean_x), mean_x));
  float       sa = 0.f, sg = 0.f, da = 0.f, dg = 0.f;
  for (uint32_t i = 0; i != n; ++i) {
    sa = __fadd_rn(sa, abs_[i]);
    sg = __fadd_rn(sg, arg[i]);
    da = __fadd_rn(da, __fmul_rn(abs_[i], (float)i));
    dg = __fadd_rn(dg, __fmul_rn(arg[i], (float)i));
  }
  const float mean_abs = __fdiv_rn(sa, nf), mean_arg = __fdiv_rn(sg, nf);
  VirtualPilotFit f;
  f.slope_abs = __fdiv_rn(__fsub_rn(da, __fmul_rn(__fmul_rn(mean_x, mean_abs), nf)), den);
  f.slope_arg = __fdiv_rn(__fsub_rn(dg, __fmul_rn(__fmul_rn(mean_x, mean_arg), nf)), den);
  f.icp_abs   = __fsub_rn(mean_abs, __fmul_rn(f.slope_abs, mean_x));
  f.icp_arg   = __fsub_rn(mean_arg, __fmul_rn(f.slope_arg, mean_x));
  return f;
}

__device__ __forceinline__ float2 virtual_pilot_value(const VirtualPilotFit& f, int position)
{
  const float  x = (float)position;
  const float  r = __fadd_rn(__fmul_rn(f.slope_abs, x), f.icp_abs);
  const float2 e = phasor(__fadd_rn(__fmul_rn(f.slope_arg, x), f.icp_arg));
  return make_float2(__fmul_rn(r, e.x), __fmul_rn(r, e.y));
}

__device__ inline void virtual_pilots(const float* abs_, float* arg, uint32_t n, int offset, float2* out)
{
  const VirtualPilotFit f = virtual_pilot_fit(abs_, arg, n);
  for (uint32_t i = 0; i != n; ++i) {
    out[i] = virtual_pilot_value(f, (int)i + offset);
  }
}

// What compute() derives from a (port, layer)'s sums: the noise variance floored at rsrp / 1e10, the SNR, the time alignment of
// a signed inverse-DFT bin and the CFO in Hz (NaN where there is none).
__device__ __forceinline__ nrphy_pusch_chest_meas_t chest_measurements(float rsrp, float epre, float nvar_raw, float beta, int ta_bins,
                                                                      bool has_cfo, float cfo, uint32_t scs_hz)
{
  const float min_noise = __fdiv_rn(rsrp, 1e10f);
  const float noise_var = nvar_raw > min_noise ? nvar_raw : min_noise;
  const float datarp    = __fdiv_rn(__fdiv_rn(rsrp, beta), beta);
  nrphy_pusch_chest_meas_t m;
  m.noise_var = noise_var;
  m.rsrp      = rsrp;
  m.epre      = epre;
  m.snr       = noise_var != 0.f ? __fdiv_rn(datarp, noise_var) : 1000.f;
  m.ta_s      = (float)((double)ta_bins / (4096.0 * (double)scs_hz));
  m.ta_bins   = ta_bins;
  m.cfo_hz    = has_cfo ? __fmul_rn(__fmul_rn(cfo, (float)(scs_hz / 1000u)), 1000.f) : __builtin_nanf("");
  m.reserved_ = 0;
  return m;
}

} // namespace
} // namespace nrphy
