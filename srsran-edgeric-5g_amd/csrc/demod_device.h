// Soft demapping arithmetic of the reference's demodulation mapper, per symbol, shared by the kernels that demodulate: the
// soft demodulator (demod_kernels.hip) and the PUSCH demodulator (pusch_demod_kernels.hip), so that both give the same soft
// bits for the same symbol at the same position of its span.  See demod_kernels.hip for what the two arithmetics are.
#pragma once

#include "nrphy_internal.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr float NEAR_ZERO = 1e-9f;
constexpr float LLR_MAXF  = 120.f;

// log_likelihood_ratio::quantize (R/lib/phy/upper/log_likelihood_ratio.cpp:89-98): round half away from zero.
__device__ __forceinline__ int quantize_generic(float value, float range)
{
  const float clipped = fabsf(value) > range ? copysignf(range, value) : value;
  return (int)roundf(__fmul_rn(__fdiv_rn(clipped, range), LLR_MAXF));
}
// mm256::quantize_ps (R/lib/phy/upper/channel_modulation/avx2_helpers.h:118-170): scale, clip, nearest even, NaN -> 0.
__device__ __forceinline__ int quantize_vector(float value, float scale /* 120 / range */)
{
  const float v = __fmul_rn(value, scale);
  const float c = __builtin_fmaxf(-LLR_MAXF, __builtin_fminf(v, LLR_MAXF)); // v_med3_f32; a NaN is replaced below
  return v != v ? 0 : (int)rintf(c);
}

__device__ __forceinline__ float safe_rcp(float noise)
{
  return noise > 0.f ? __fdiv_rn(1.0f, noise) : 0.f;
}

struct Tables {
  float2 line[DEMOD_MAX_PAIRS][16]; // (slope, intercept) of an interval: one 8-byte LDS read per soft bit
};

// The soft bits of a thread (up to 16) collected in registers: byte k of the thread's output.  Every index is a compile-time
// constant after unrolling (a byte array here ends up in LDS, one ds_write_b8 per soft bit).
struct LlrBytes {
  uint32_t w[4] = {0, 0, 0, 0};
  __device__ __forceinline__ void put(uint32_t k, int v) { w[k >> 2] |= ((uint32_t)v & 0xFFu) << (8u * (k & 3u)); }
  __device__ __forceinline__ uint8_t get(uint32_t k) const { return (uint8_t)(w[k >> 2] >> (8u * (k & 3u))); }
};

// One component (real or imaginary part) of a table-driven constellation, bit pair `pair`.  VECTOR: the reference's AVX2
// arithmetic (reciprocal width, nearest-even quantiser), else its generic one.
template <bool VECTOR>
__device__ __forceinline__ int interval_llr(const DemodLaunch& p, const Tables& t, uint32_t pair, float v, float rcp)
{
  const int    n    = (int)p.nof_intervals[pair];
  const float  pos  = VECTOR ? __fmul_rn(v, p.rcp_width[pair]) : __fdiv_rn(v, p.width[pair]);
  const int    idx  = max(0, min((int)floorf(pos) + n / 2, n - 1));
  const float2 line = t.line[pair][idx];
  const float  l    = __fmul_rn(__fmaf_rn(line.x, v, line.y), rcp);
  if (VECTOR) {
    return quantize_vector(fabsf(v) <= NEAR_ZERO ? 0.f : l, p.scale);
  }
  return quantize_generic(l, p.range);
}

// The soft bits of symbol i of its span into bytes [at, at + qm) of out.  The kernel is specialised per modulation (no run-time
// switch, the bit-pair loop unrolled) and per arithmetic: a thread whose symbols all lie in the span's vector part -- every
// thread but the last few of a span -- runs the VECTOR copy.
template <uint32_t MOD, bool VECTOR>
__device__ __forceinline__ void demodulate_symbol(const DemodLaunch& p, const Tables& t, uint32_t i, float re, float im, float noise,
                                                  LlrBytes& out, uint32_t at)
{
  constexpr float GAIN_PSK = 2.0f * 1.41421356237309504880f;
  if constexpr (MOD == NRPHY_MOD_BPSK || MOD == NRPHY_MOD_PI2_BPSK) {
    // pi/2-BPSK: odd symbols are rotated by -90 degrees first, (im, -re)
    const bool  rot = MOD == NRPHY_MOD_PI2_BPSK && (i & 1u);
    const float a = rot ? im : re, b = rot ? -re : im;
    out.put(at, !(noise > 0.f) ? 0 : quantize_generic(__fdiv_rn(__fmul_rn(GAIN_PSK, __fadd_rn(a, b)), noise), p.range));
  } else if constexpr (MOD == NRPHY_MOD_QPSK) {
#pragma unroll
    for (uint32_t c = 0; c != 2; ++c) {
      const float v = c ? im : re;
      if (VECTOR) {
        out.put(at + c, quantize_vector(__fmul_rn(__fmul_rn(GAIN_PSK, v), safe_rcp(noise)), p.scale));
      } else {
        out.put(at + c, !(noise > 0.f) ? 0 : quantize_generic(__fdiv_rn(__fmul_rn(GAIN_PSK, v), noise), p.range));
      }
    }
  } else if constexpr (MOD == NRPHY_MOD_QAM16) {
    const float g1 = p.qam16_gain, thr = p.qam16_threshold;
    const bool  blank = !VECTOR && __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)) < NEAR_ZERO;
#pragma unroll
    for (uint32_t c = 0; c != 2; ++c) {
      const float v     = c ? im : re;
      const float first = __fmul_rn(g1, v);
      // 2 * first is exact, so the reference's contracted and uncontracted forms agree
      const float l01 = fabsf(v) > thr ? __fsub_rn(__fmul_rn(2.0f, first), copysignf(0.8f, v)) : first;
      if (VECTOR) {
        const float rcp  = safe_rcp(noise);
        const bool  zero = fabsf(v) <= NEAR_ZERO;
        out.put(at + c, quantize_vector(zero ? 0.f : __fmul_rn(l01, rcp), p.scale));
        out.put(at + 2u + c, quantize_vector(zero ? 0.f : __fmul_rn(__fsub_rn(0.8f, fabsf(first)), rcp), p.scale));
      } else if (!(blank || !(noise > 0.f))) {
        out.put(at + c, quantize_generic(__fdiv_rn(l01, noise), p.range));
        out.put(at + 2u + c, quantize_generic(__fdiv_rn(__fmaf_rn(-g1, fabsf(v), 0.8f), noise), p.range)); // contracted there
      }
    }
  } else { // 64-QAM, 256-QAM
    constexpr uint32_t pairs = MOD / 2u;
    const float        rcp   = safe_rcp(noise);
    const bool         blank = !VECTOR && __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)) < NEAR_ZERO;
#pragma unroll
    for (uint32_t k = 0; k != pairs; ++k) {
      out.put(at + 2u * k, blank ? 0 : interval_llr<VECTOR>(p, t, k, re, rcp));
      out.put(at + 2u * k + 1u, blank ? 0 : interval_llr<VECTOR>(p, t, k, im, rcp));
    }
  }
}

} // namespace
} // namespace nrphy
