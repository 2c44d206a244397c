// The channel equaliser's per-RE arithmetic, shared by the kernels that equalise: the PUSCH demodulator and the standalone
// equaliser (pusch_demod_kernels.hip), the PUCCH format 1 detector (pucch_kernels.hip) and the PUCCH format 2 receiver
// (pucch2_kernels.hip).  One function, so that every caller gets the same bits.  is_normal and the infinity are exact_device.h's.
#pragma once

#include "bits_device.h"
#include "exact_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {

// One RE of channel_equalizer::equalize, the reference's scalar arithmetic operation by operation (std::complex products written
// out: (a + jb) conj(c + jd) = (ac + bd) + j(bc - ad)), contraction off, exact division.  y[i]: received word of receive port i;
// h[l][i]: estimate of layer l at port i; nv[i]: port noise variances; nv_max: their maximum (std::max_element).  Out: symbol and
// noise variance per layer.
__device__ __forceinline__ void equalize_re(uint32_t algorithm, uint32_t nof_layers, uint32_t nof_ports, const uint32_t (&y)[NRPHY_MAX_PORTS],
                                            const uint32_t (&h)[2][NRPHY_MAX_PORTS], const float (&nv)[NRPHY_MAX_PORTS], float nv_max,
                                            float tx_scaling, float2 (&x)[2], float (&v)[2])
{
  x[0] = x[1] = make_float2(0.f, 0.f);
  v[0] = v[1] = F_INF;
  if (nof_layers == 1) {
    // ZF: equalize_zf_single_tx_layer_reduction drops the ports whose variance is not in (0, inf), then equalize_zf_1xn checks
    // every RE and port as MMSE does; together: a port counts where |h|^2 and its variance are normal and the variance positive.
    const bool mmse   = algorithm == NRPHY_EQ_MMSE;
    float      msq    = 0.f, nacc = 0.f;
    float2     acc    = make_float2(0.f, 0.f);
#pragma unroll
    for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
      if (i < nof_ports) {
        const float2 r  = cbf16_to_float2(y[i]);
        float2       c  = cbf16_to_float2(h[0][i]);
        if (mmse) {
          c = make_float2(__fmul_rn(c.x, tx_scaling), __fmul_rn(c.y, tx_scaling));
        }
        const float n = __fadd_rn(__fmul_rn(c.x, c.x), __fmul_rn(c.y, c.y));
        if (is_normal(n) && is_normal(nv[i]) && nv[i] > 0.f) {
          msq   = __fadd_rn(msq, n);
          nacc  = __fadd_rn(nacc, __fmul_rn(n, nv[i]));
          acc.x = __fadd_rn(acc.x, __fadd_rn(__fmul_rn(r.x, c.x), __fmul_rn(r.y, c.y)));
          acc.y = __fadd_rn(acc.y, __fsub_rn(__fmul_rn(r.y, c.x), __fmul_rn(r.x, c.y)));
        }
      }
    }
    if (mmse) {
      if (is_normal(msq) && is_normal(nacc)) {
        const float rcp = __fdiv_rn(1.0f, __fadd_rn(__fmul_rn(msq, msq), nacc));
        x[0]            = make_float2(__fmul_rn(__fmul_rn(acc.x, msq), rcp), __fmul_rn(__fmul_rn(acc.y, msq), rcp));
        v[0]            = __fmul_rn(nacc, rcp);
      }
    } else {
      const float d = __fmul_rn(tx_scaling, msq);
      if (is_normal(d) && is_normal(nacc)) {
        const float rcp = __fdiv_rn(1.0f, d);
        x[0]            = make_float2(__fmul_rn(acc.x, rcp), __fmul_rn(acc.y, rcp));
        v[0]            = __fmul_rn(__fmul_rn(nacc, rcp), rcp);
      }
    }
    return;
  }
  // ZF, two layers (equalize_zf_2xn): H^H H = [n0 xi; conj(xi) n1], matched filter m = H^H y.
  float  n0 = 0.f, n1 = 0.f;
  float2 xi = make_float2(0.f, 0.f), m0 = make_float2(0.f, 0.f), m1 = make_float2(0.f, 0.f);
#pragma unroll
  for (uint32_t i = 0; i != NRPHY_MAX_PORTS; ++i) {
    if (i < nof_ports) {
      const float2 r = cbf16_to_float2(y[i]), c0 = cbf16_to_float2(h[0][i]), c1 = cbf16_to_float2(h[1][i]);
      n0   = __fadd_rn(n0, __fadd_rn(__fmul_rn(c0.x, c0.x), __fmul_rn(c0.y, c0.y)));
      n1   = __fadd_rn(n1, __fadd_rn(__fmul_rn(c1.x, c1.x), __fmul_rn(c1.y, c1.y)));
      xi.x = __fadd_rn(xi.x, __fadd_rn(__fmul_rn(c0.x, c1.x), __fmul_rn(c0.y, c1.y)));
      xi.y = __fadd_rn(xi.y, __fsub_rn(__fmul_rn(c0.x, c1.y), __fmul_rn(c0.y, c1.x)));
      m0.x = __fadd_rn(m0.x, __fadd_rn(__fmul_rn(c0.x, r.x), __fmul_rn(c0.y, r.y)));
      m0.y = __fadd_rn(m0.y, __fsub_rn(__fmul_rn(c0.x, r.y), __fmul_rn(c0.y, r.x)));
      m1.x = __fadd_rn(m1.x, __fadd_rn(__fmul_rn(c1.x, r.x), __fmul_rn(c1.y, r.y)));
      m1.y = __fadd_rn(m1.y, __fsub_rn(__fmul_rn(c1.x, r.y), __fmul_rn(c1.y, r.x)));
    }
  }
  const float xi_sq  = __fadd_rn(__fmul_rn(xi.x, xi.x), __fmul_rn(xi.y, xi.y));
  const float d_pinv = __fmul_rn(tx_scaling, __fsub_rn(__fmul_rn(n0, n1), xi_sq));
  const float d_nv   = __fmul_rn(tx_scaling, d_pinv);
  if (is_normal(d_pinv)) {
    const float rcp = __fdiv_rn(1.0f, d_pinv), nrcp = __fdiv_rn(1.0f, d_nv);
    // (n1 m0 - xi m1) / d and (n0 m1 - conj(xi) m0) / d
    const float a0 = __fsub_rn(__fmul_rn(n1, m0.x), __fsub_rn(__fmul_rn(xi.x, m1.x), __fmul_rn(xi.y, m1.y)));
    const float b0 = __fsub_rn(__fmul_rn(n1, m0.y), __fadd_rn(__fmul_rn(xi.x, m1.y), __fmul_rn(xi.y, m1.x)));
    const float a1 = __fsub_rn(__fmul_rn(n0, m1.x), __fadd_rn(__fmul_rn(xi.x, m0.x), __fmul_rn(xi.y, m0.y)));
    const float b1 = __fsub_rn(__fmul_rn(n0, m1.y), __fsub_rn(__fmul_rn(xi.x, m0.y), __fmul_rn(xi.y, m0.x)));
    x[0]           = make_float2(__fmul_rn(a0, rcp), __fmul_rn(b0, rcp));
    x[1]           = make_float2(__fmul_rn(a1, rcp), __fmul_rn(b1, rcp));
    v[0]           = __fmul_rn(__fmul_rn(nv_max, n1), nrcp);
    v[1]           = __fmul_rn(__fmul_rn(nv_max, n0), nrcp);
  }
}

// std::max_element over the first n variances (the first of equal maxima; a leading NaN stays).
__device__ __forceinline__ float max_noise(const float (&nv)[NRPHY_MAX_PORTS], uint32_t n)
{
  float m = nv[0];
#pragma unroll
  for (uint32_t i = 1; i != NRPHY_MAX_PORTS; ++i) {
    if (i < n && m < nv[i]) {
      m = nv[i];
    }
  }
  return m;
}

} // namespace nrphy
