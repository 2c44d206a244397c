// The exactly rounded float arithmetic of the uplink receivers, each operation defined once so that every kernel rounds alike:
// the reference's constants, std::complex<float> and srsvec products written out per component, transcendentals evaluated in
// double and rounded once, the time-alignment search's comparison rule and the merge of the ports' measurements.  Contraction is
// off; the only fused multiply-adds are dft_accumulate's.  Included by chest_device.h and equalize_device.h, and directly by the
// receivers that need neither (pusch_proc_kernels.hip, prach_kernels.hip).
#pragma once

#include "bits_device.h"

#include <hip/hip_runtime.h>
#include <limits>

namespace nrphy {

constexpr float TWOPI_F        = 6.28318548f; // 2.0F * static_cast<float>(M_PI)
constexpr float PI_F           = 3.14159274f;
constexpr float SQRT1_2_F      = 0.707106769f;
constexpr float FLT_NORMAL_MIN = 1.17549435e-38f;
constexpr float FLT_LARGEST    = 3.40282347e+38f;
constexpr float F_INF          = __builtin_huge_valf();
static_assert(FLT_NORMAL_MIN == std::numeric_limits<float>::min() && FLT_LARGEST == std::numeric_limits<float>::max(),
              "the bounds of std::isnormal");

// A receiver multiplies with exact::cmul, never with fft_device.h's cmul(cf, cf): that one is packed and fused for the transforms
// and rounds differently from the reference's std::complex<float>.
namespace exact {

// (a + jb)(c + jd) as std::complex<float> and srsvec::prod write it.
__device__ __forceinline__ float2 cmul(float2 x, float2 h)
{
  return make_float2(__fsub_rn(__fmul_rn(x.x, h.x), __fmul_rn(x.y, h.y)), __fadd_rn(__fmul_rn(x.x, h.y), __fmul_rn(x.y, h.x)));
}

// y conj(p) (srsvec::prod_conj; a term of srsvec::dot_prod).
__device__ __forceinline__ float2 mul_conj(float2 y, float2 p)
{
  return make_float2(__fadd_rn(__fmul_rn(y.x, p.x), __fmul_rn(y.y, p.y)), __fsub_rn(__fmul_rn(y.y, p.x), __fmul_rn(y.x, p.y)));
}

// |v|^2 (std::norm).
__device__ __forceinline__ float norm(float2 v)
{
  return __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
}

} // namespace exact

// std::polar(1.0F, x) with cos and sin evaluated in double and rounded once.
__device__ __forceinline__ float2 phasor(float x)
{
  return make_float2((float)cos((double)x), (float)sin((double)x));
}

// complex_exponential_table(size, 1)[index]: polar(1, float(2 pi) float(index) / float(size)), the angle in single precision.
__device__ __forceinline__ float2 unit_circle(uint32_t index, uint32_t size)
{
  return phasor(__fdiv_rn(__fmul_rn(TWOPI_F, (float)index), (float)size));
}

// convert_power_to_dB: log10 in double, rounded once.
__device__ __forceinline__ float to_dB(float v)
{
  return __fmul_rn(10.0f, (float)log10((double)v));
}

// std::isnormal: false for zero, subnormals, infinities and NaN.
__device__ __forceinline__ bool is_normal(float x)
{
  const float a = fabsf(x);
  return a >= FLT_NORMAL_MIN && a <= FLT_LARGEST;
}

__device__ __forceinline__ uint32_t to_cbf16(float re, float im)
{
  return to_bf16_bits(re) | (to_bf16_bits(im) << 16);
}

// The QPSK pilot of bits b and b + 1 of the Gold words c(0 ...), first bit in the word's top bit; b is even, so both bits are in
// one word.
__device__ __forceinline__ float2 qpsk_pilot(const uint32_t* words, uint32_t b)
{
  const uint32_t w0 = words[b >> 5];
  const uint32_t c0 = (w0 >> (31u - (b & 31u))) & 1u, c1 = (w0 >> (30u - (b & 31u))) & 1u;
  return make_float2(c0 ? -SQRT1_2_F : SQRT1_2_F, c1 ? -SQRT1_2_F : SQRT1_2_F);
}

// ---- the time-alignment search (time_alignment_estimator_dft_impl::estimate) ------------------------------------------------
// acc += v t, one term of the direct partial inverse DFT: fused, because |acc|^2 feeds a comparison and nothing else.
__device__ __forceinline__ void dft_accumulate(float2& acc, float2 v, float2 t)
{
  acc.x = __fmaf_rn(v.x, t.x, __fmaf_rn(-v.y, t.y, acc.x));
  acc.y = __fmaf_rn(v.x, t.y, __fmaf_rn(v.y, t.x, acc.y));
}

// The larger of two (magnitude, bin) candidates; the lower bin on equal magnitudes (max_abs_element returns the first maximum).
// A scan in ascending bin order may use it as it stands: there it is the strict comparison.
__device__ __forceinline__ void take_max(float& m, uint32_t& i, float m2, uint32_t i2)
{
  if (m2 > m || (m2 == m && i2 < i)) {
    m = m2;
    i = i2;
  }
}

// The wave's best candidate of the delays (d) and of the advances (a); every lane gets both.
__device__ __forceinline__ void wave_take_max(float& best_d, uint32_t& id, float& best_a, uint32_t& ia)
{
#pragma unroll
  for (int o = WAVE / 2; o != 0; o >>= 1) {
    take_max(best_d, id, __shfl_xor(best_d, o), __shfl_xor(id, o));
    take_max(best_a, ia, __shfl_xor(best_a, o), __shfl_xor(ia, o));
  }
}

// The signed bin: the delay wins against an equal advance; ia counts from the start of the last `window` bins.
__device__ __forceinline__ int ta_signed_bin(float best_d, uint32_t id, float best_a, uint32_t ia, uint32_t window)
{
  return best_d >= best_a ? (int)id : (int)ia - (int)window;
}

// ---- channel_estimate::get_channel_state_information over layer 0 of the receive ports ----------------------------------------
// add() the ports in port order: the sums are float sums in that order, and best_rx_port starts at port 0 and moves on a
// strictly better SNR only.
struct CsiMerge {
  float epre_lin = 0.f, rsrp_lin = 0.f, noise_lin = 0.f, best_snr = 0.f;
  float ta_s = 0.f, cfo_hz = 0.f; // the best port's

  __device__ __forceinline__ void add(uint32_t port, float noise_var, float rsrp, float epre, float snr, float port_ta_s, float port_cfo_hz)
  {
    epre_lin  = __fadd_rn(epre_lin, epre);
    rsrp_lin  = __fadd_rn(rsrp_lin, rsrp);
    noise_lin = __fadd_rn(noise_lin, noise_var);
    if (port == 0 || snr > best_snr) {
      ta_s   = port_ta_s;
      cfo_hz = port_cfo_hz;
    }
    if (snr > best_snr) {
      best_snr = snr;
    }
  }
  // get_layer_average_snr(0): 1e6 where the noise sum is not normal.
  __device__ __forceinline__ float sinr_dB() const { return to_dB(is_normal(noise_lin) ? __fdiv_rn(rsrp_lin, noise_lin) : 1e6f); }
  __device__ __forceinline__ float rsrp_dB(uint32_t nof_ports) const { return to_dB(__fdiv_rn(rsrp_lin, (float)nof_ports)); }
  __device__ __forceinline__ float epre_dB(uint32_t nof_ports) const { return to_dB(__fdiv_rn(epre_lin, (float)nof_ports)); }
};

} // namespace nrphy
