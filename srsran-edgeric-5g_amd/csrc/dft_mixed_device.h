// Run-time mixed-radix Stockham transform in LDS for gfx950: the inverse DFT of the transform-precoding sizes N = 12 * M_rb =
// 2^a 3^b 5^c (53 of them, 12 to 3240 points), one workgroup of MIXED_DFT_THREADS threads per transform.  fft_device.h's plans
// are compile-time radix lists for 18 sizes; here the stage list (radices of {2, 3, 4, 5}, built on the host: MixedDftPlan)
// is read from the launch descriptor, and one routine serves every size.  Both the stand-alone kernel
// (transform_precoder_kernels.hip) and the fused PUSCH demodulator (pusch_demod_kernels.hip) call mixed_dft_inverse(), with the
// same thread count, so the same input gives the same bits in both.
//
// A stage of radix R over sub-transforms of ns points (ns = the product of the earlier radices): butterfly j < N / R reads
// in[j + r N / R], multiplies by exp(+2 pi i r k / (ns R)), k = j mod ns -- element r k N / (ns R) < N of the size's table, every
// twiddle rounded once from double --, and writes out[(j - k) R + k + r ns].  After the last stage the result is in natural order.
// The two buffers alternate; a workgroup barrier separates the stages.
#pragma once

#include "fft_device.h"

namespace nrphy {

// Radix 5: y0 = a0 + t1 + t2, y1,4 = (a0 + c1 t1 + c2 t2) +- SIGN j (s1 d1 + s2 d2), y2,3 = (a0 + c2 t1 + c1 t2) +- SIGN j
// (s2 d1 - s1 d2) with t1 = a1 + a4, t2 = a2 + a3, d1 = a1 - a4, d2 = a2 - a3.
template <int SIGN>
__device__ __forceinline__ void dft5(cf& a0, cf& a1, cf& a2, cf& a3, cf& a4)
{
  constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
  constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
  const cf        t1 = cadd(a1, a4), t2 = cadd(a2, a3), d1 = csub(a1, a4), d2 = csub(a2, a3);
  const cf        m1 = (a0 + c1 * t1) + c2 * t2, m2 = (a0 + c2 * t1) + c1 * t2;
  const cf        n1 = s1 * d1 + s2 * d2, n2 = s2 * d1 - s1 * d2;
  a0                 = cadd(a0, cadd(t1, t2));
  a1                 = add_sjb<SIGN>(m1, n1);
  a4                 = sub_sjb<SIGN>(m1, n1);
  a2                 = add_sjb<SIGN>(m2, n2);
  a3                 = sub_sjb<SIGN>(m2, n2);
}
template <int SIGN>
struct Butterfly<SIGN, 5> {
  static __device__ __forceinline__ void run(cf (&a)[5]) { dft5<SIGN>(a[0], a[1], a[2], a[3], a[4]); }
};

template <int R>
__device__ __forceinline__ void mixed_dft_stage(const cf* in, cf* out, const float2* __restrict__ tw, uint32_t n, uint32_t ns,
                                                uint32_t tid)
{
  const uint32_t m = n / (uint32_t)R, step = m / ns; // butterflies of the stage; table elements per unit of r k
  for (uint32_t j = tid; j < m; j += MIXED_DFT_THREADS) {
    const uint32_t k = j % ns;
    cf             a[R];
#pragma unroll
    for (int r = 0; r != R; ++r) {
      a[r] = in[j + (uint32_t)r * m];
    }
    if (ns != 1u) { // workgroup-uniform: the first stage has no twiddles
#pragma unroll
      for (int r = 1; r != R; ++r) {
        const float2 w = tw[(uint32_t)r * k * step];
        a[r]           = cmul(a[r], make_cf(w.x, w.y));
      }
    }
    Butterfly<+1, R>::run(a);
    const uint32_t o = (j - k) * (uint32_t)R + k;
#pragma unroll
    for (int r = 0; r != R; ++r) {
      out[o + (uint32_t)r * ns] = a[r];
    }
  }
}

// The unnormalised inverse DFT of a[0, p.n).  Every thread of the workgroup (MIXED_DFT_THREADS of them) calls it; the caller's
// writes to `a` need no barrier of their own.  Returns the buffer that holds the result, `a` or `b`, after a barrier: the
// other one is free.
__device__ inline cf* mixed_dft_inverse(const MixedDftPlan& p, cf* a, cf* b, uint32_t tid)
{
  __syncthreads();
  uint32_t ns = 1;
  for (uint32_t s = 0; s != p.nof_stages; ++s) { // workgroup-uniform
    const uint32_t r = p.radix[s];
    switch (r) {
      case 2:
        mixed_dft_stage<2>(a, b, p.twiddle, p.n, ns, tid);
        break;
      case 3:
        mixed_dft_stage<3>(a, b, p.twiddle, p.n, ns, tid);
        break;
      case 4:
        mixed_dft_stage<4>(a, b, p.twiddle, p.n, ns, tid);
        break;
      default:
        mixed_dft_stage<5>(a, b, p.twiddle, p.n, ns, tid);
        break;
    }
    __syncthreads();
    ns *= r;
    cf* t = a;
    a     = b;
    b     = t;
  }
  return a;
}

} // namespace nrphy
