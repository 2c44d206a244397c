// Stockham transforms in LDS for gfx950: packed-FP32 complex arithmetic, the register butterflies, the radix plans and the
// stages, shared by the OFDM / DFT kernels (ofdm_kernels.hip) and the PRACH detector (prach_kernels.hip).  A transform of N
// points runs on Plan<N>::T threads of a workgroup; the caller owns the LDS buffer of N + N / 16 + 16 elements.
#pragma once

#include "bits_device.h"

#include <type_traits>

namespace nrphy {

template <uint32_t V>
using Const = std::integral_constant<uint32_t, V>;

// f(Const<0>{}), ..., f(Const<COUNT - 1>{}): a loop whose index is a compile-time constant inside the body.
template <class F, uint32_t... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<uint32_t, I...>)
{
  (f(Const<I>{}), ...);
}
template <uint32_t COUNT, class F>
__device__ __forceinline__ void static_for(F&& f)
{
  static_for_impl(f, std::make_integer_sequence<uint32_t, COUNT>{});
}

// ---- complex arithmetic on packed FP32 ------------------------------------------------------------------------
// A complex number is one 64-bit VGPR pair (re, im) and every operation below is one or two v_pk_*_f32
// instructions.  hipcc pairs scalar float code into packed instructions on its own, but it cannot negate or swap one
// half of an operand (it emits both variants and v_mov's the halves back together), so the operations that need
// op_sel / neg_lo / neg_hi are written out: the register butterflies are VALU-bound, not memory-bound.
typedef float cf __attribute__((ext_vector_type(2)));

__device__ __forceinline__ cf cadd(cf a, cf b)
{
  return a + b;
}
__device__ __forceinline__ cf csub(cf a, cf b)
{
  return a - b;
}
// a * b:  t = (a.im b.im, a.re b.im);  result = (a.re b.re - t.lo, a.im b.re + t.hi).
__device__ __forceinline__ cf cmul(cf a, cf b)
{
  cf t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
  return r;
}
// The same with a wave-uniform b held in an SGPR pair (constants, the per-symbol phase).
__device__ __forceinline__ cf cmul_uniform(cf a, cf b)
{
  cf t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "s"(b));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] neg_lo:[0,0,1]" : "=v"(r) : "v"(a), "s"(b), "v"(t));
  return r;
}
// a + j b = (a.re - b.im, a.im + b.re) and a - j b = (a.re + b.im, a.im - b.re).
__device__ __forceinline__ cf add_jb(cf a, cf b)
{
  cf r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ cf sub_jb(cf a, cf b)
{
  cf r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// a + SIGN j b, a - SIGN j b (SIGN = +1: inverse transform, -1: direct).
template <int SIGN>
__device__ __forceinline__ cf add_sjb(cf a, cf b)
{
  return SIGN > 0 ? add_jb(a, b) : sub_jb(a, b);
}
template <int SIGN>
__device__ __forceinline__ cf sub_sjb(cf a, cf b)
{
  return SIGN > 0 ? sub_jb(a, b) : add_jb(a, b);
}
__device__ __forceinline__ cf make_cf(float re, float im)
{
  cf r = {re, im};
  return r;
}

// ---- register butterflies: a[k] <- sum_n a[n] * exp(SIGN * 2 pi i n k / R), natural order in and out ---------
template <int SIGN>
__device__ __forceinline__ void dft2(cf& a0, cf& a1)
{
  cf t = a0;
  a0   = cadd(t, a1);
  a1   = csub(t, a1);
}

// ROT2: input a2 still has to be multiplied by SIGN j (a twiddle of the enclosing transform, folded in for free).
template <int SIGN, bool ROT2 = false>
__device__ __forceinline__ void dft4(cf& a0, cf& a1, cf& a2, cf& a3)
{
  cf p0 = ROT2 ? add_sjb<SIGN>(a0, a2) : cadd(a0, a2);
  cf q0 = ROT2 ? sub_sjb<SIGN>(a0, a2) : csub(a0, a2);
  cf p1 = cadd(a1, a3), d = csub(a1, a3);
  a0    = cadd(p0, p1);
  a1    = add_sjb<SIGN>(q0, d);
  a2    = csub(p0, p1);
  a3    = sub_sjb<SIGN>(q0, d);
}

template <int SIGN, int R>
struct Butterfly;

template <int SIGN>
struct Butterfly<SIGN, 2> {
  static __device__ __forceinline__ void run(cf (&a)[2]) { dft2<SIGN>(a[0], a[1]); }
};
template <int SIGN>
struct Butterfly<SIGN, 4> {
  static __device__ __forceinline__ void run(cf (&a)[4]) { dft4<SIGN>(a[0], a[1], a[2], a[3]); }
};
template <int SIGN>
struct Butterfly<SIGN, 8> {
  // 8 = 2 x 4: X[k1 + 2 k2] = sum_{n2<4} W8^(n2 k1) W4^(n2 k2) [ sum_{n1<2} x[4 n1 + n2] W2^(n1 k1) ].
  static __device__ __forceinline__ void run(cf (&a)[8])
  {
    constexpr float h = 0.70710678118654752440f;
    dft2<SIGN>(a[0], a[4]);
    dft2<SIGN>(a[1], a[5]);
    dft2<SIGN>(a[2], a[6]);
    dft2<SIGN>(a[3], a[7]);
    // k1 = 1 row: multiply by W8^n2, n2 = 1, 2, 3 (n2 = 2 is SIGN j, folded into the butterfly).
    a[5] = cmul_uniform(a[5], make_cf(h, SIGN * h));
    a[7] = cmul_uniform(a[7], make_cf(-h, SIGN * h));
    dft4<SIGN>(a[0], a[1], a[2], a[3]);       // k1 = 0: X[0], X[2], X[4], X[6]
    dft4<SIGN, true>(a[4], a[5], a[6], a[7]); // k1 = 1: X[1], X[3], X[5], X[7]
    cf x1 = a[4], x2 = a[1], x3 = a[5], x4 = a[2], x5 = a[6], x6 = a[3];
    a[1] = x1;
    a[2] = x2;
    a[3] = x3;
    a[4] = x4;
    a[5] = x5;
    a[6] = x6;
  }
};
template <int SIGN>
struct Butterfly<SIGN, 16> {
  // 16 = 4 x 4: X[k1 + 4 k2] = sum_{n2<4} W16^(n2 k1) W4^(n2 k2) [ sum_{n1<4} x[4 n1 + n2] W4^(n1 k1) ].
  static __device__ __forceinline__ void run(cf (&a)[16])
  {
    constexpr float c1 = 0.92387953251128675613f, s1 = 0.38268343236508977173f, h = 0.70710678118654752440f;
    // Inner transforms over n1 (stride 4) for each n2; result index k1 replaces n1.
    dft4<SIGN>(a[0], a[4], a[8], a[12]);
    dft4<SIGN>(a[1], a[5], a[9], a[13]);
    dft4<SIGN>(a[2], a[6], a[10], a[14]);
    dft4<SIGN>(a[3], a[7], a[11], a[15]);
    // Twiddles W16^(n2 k1) on element a[4 k1 + n2]; W16^4 = SIGN j on a[10] is folded into its butterfly.
    a[5]  = cmul_uniform(a[5], make_cf(c1, SIGN * s1));    // 1*1
    a[6]  = cmul_uniform(a[6], make_cf(h, SIGN * h));      // 2*1
    a[7]  = cmul_uniform(a[7], make_cf(s1, SIGN * c1));    // 3*1
    a[9]  = cmul_uniform(a[9], make_cf(h, SIGN * h));      // 1*2
    a[11] = cmul_uniform(a[11], make_cf(-h, SIGN * h));    // 3*2
    a[13] = cmul_uniform(a[13], make_cf(s1, SIGN * c1));   // 1*3
    a[14] = cmul_uniform(a[14], make_cf(-h, SIGN * h));    // 2*3
    a[15] = cmul_uniform(a[15], make_cf(-c1, -SIGN * s1)); // 3*3 = 9 -> W16^9
    // Outer transforms over n2 for each k1; result a[4 k1 + k2] = X[k1 + 4 k2].
    dft4<SIGN>(a[0], a[1], a[2], a[3]);
    dft4<SIGN>(a[4], a[5], a[6], a[7]);
    dft4<SIGN, true>(a[8], a[9], a[10], a[11]);
    dft4<SIGN>(a[12], a[13], a[14], a[15]);
    // Transpose 4x4 to natural order: X[k1 + 4 k2] currently at a[4 k1 + k2].
    cf t;
    t = a[1];  a[1] = a[4];   a[4] = t;
    t = a[2];  a[2] = a[8];   a[8] = t;
    t = a[3];  a[3] = a[12];  a[12] = t;
    t = a[6];  a[6] = a[9];   a[9] = t;
    t = a[7];  a[7] = a[13];  a[13] = t;
    t = a[11]; a[11] = a[14]; a[14] = t;
  }
};

// Radix 3: y0 = a0 + (a1 + a2), y1,2 = a0 - (a1 + a2) / 2 +- SIGN j (sqrt(3) / 2) (a1 - a2).
template <int SIGN>
__device__ __forceinline__ void dft3(cf& a0, cf& a1, cf& a2)
{
  constexpr float s = 0.86602540378443864676f;
  const cf        t = cadd(a1, a2), d = csub(a1, a2);
  const cf        u = a0 - 0.5f * t, v = s * d;
  a0                = cadd(a0, t);
  a1                = add_sjb<SIGN>(u, v);
  a2                = sub_sjb<SIGN>(u, v);
}
template <int SIGN>
struct Butterfly<SIGN, 3> {
  static __device__ __forceinline__ void run(cf (&a)[3]) { dft3<SIGN>(a[0], a[1], a[2]); }
};
template <int SIGN>
struct Butterfly<SIGN, 6> {
  // 6 = 2 x 3: X[k1 + 2 k2] = sum_{n2<3} W6^(n2 k1) W3^(n2 k2) [ sum_{n1<2} x[3 n1 + n2] W2^(n1 k1) ].
  static __device__ __forceinline__ void run(cf (&a)[6])
  {
    constexpr float s = 0.86602540378443864676f;
    dft2<SIGN>(a[0], a[3]);
    dft2<SIGN>(a[1], a[4]);
    dft2<SIGN>(a[2], a[5]);
    a[4] = cmul_uniform(a[4], make_cf(0.5f, SIGN * s));  // W6^1
    a[5] = cmul_uniform(a[5], make_cf(-0.5f, SIGN * s)); // W6^2
    dft3<SIGN>(a[0], a[1], a[2]); // k1 = 0: X[0], X[2], X[4]
    dft3<SIGN>(a[3], a[4], a[5]); // k1 = 1: X[1], X[3], X[5]
    const cf x1 = a[3], x2 = a[1], x3 = a[4], x4 = a[2];
    a[1] = x1;
    a[2] = x2;
    a[3] = x3;
    a[4] = x4;
  }
};
template <int SIGN>
struct Butterfly<SIGN, 12> {
  // 12 = 4 x 3: X[k1 + 4 k2] = sum_{n2<3} W12^(n2 k1) W3^(n2 k2) [ sum_{n1<4} x[3 n1 + n2] W4^(n1 k1) ].
  static __device__ __forceinline__ void run(cf (&a)[12])
  {
    constexpr float s = 0.86602540378443864676f;
    dft4<SIGN>(a[0], a[3], a[6], a[9]);
    dft4<SIGN>(a[1], a[4], a[7], a[10]);
    dft4<SIGN>(a[2], a[5], a[8], a[11]);
    // Twiddles W12^(n2 k1) on a[3 k1 + n2].
    a[4]  = cmul_uniform(a[4], make_cf(s, SIGN * 0.5f));    // 1*1
    a[5]  = cmul_uniform(a[5], make_cf(0.5f, SIGN * s));    // 2*1
    a[7]  = cmul_uniform(a[7], make_cf(0.5f, SIGN * s));    // 1*2
    a[8]  = cmul_uniform(a[8], make_cf(-0.5f, SIGN * s));   // 2*2
    a[10] = cmul_uniform(a[10], make_cf(0.f, (float)SIGN)); // 1*3: SIGN j
    a[11] = make_cf(-a[11].x, -a[11].y);                    // 2*3: -1
    dft3<SIGN>(a[0], a[1], a[2]);   // k1 = 0: X[0], X[4], X[8]
    dft3<SIGN>(a[3], a[4], a[5]);   // k1 = 1: X[1], X[5], X[9]
    dft3<SIGN>(a[6], a[7], a[8]);   // k1 = 2: X[2], X[6], X[10]
    dft3<SIGN>(a[9], a[10], a[11]); // k1 = 3: X[3], X[7], X[11]
    cf x[12];
#pragma unroll
    for (int k1 = 0; k1 != 4; ++k1) {
#pragma unroll
      for (int k2 = 0; k2 != 3; ++k2) {
        x[k1 + 4 * k2] = a[3 * k1 + k2];
      }
    }
#pragma unroll
    for (int k = 0; k != 12; ++k) {
      a[k] = x[k];
    }
  }
};

// a[j] *= b^j for j = 1..R-1.  Powers are built from b^2, b^4, b^8 (squarings) so that every power is at most
// three multiplications deep (a few ulp), and applied at once to keep few values live.
template <int R>
__device__ __forceinline__ void apply_twiddle_powers(cf b, cf (&a)[R])
{
  a[1] = cmul(a[1], b);
  if constexpr (R > 2) {
    const cf b2 = cmul(b, b);
    a[2]        = cmul(a[2], b2);
    if constexpr (R > 3) {
      a[3] = cmul(a[3], cmul(b2, b));
    }
    if constexpr (R > 4) {
      const cf b4 = cmul(b2, b2);
      a[4]        = cmul(a[4], b4);
      if constexpr (R > 5) {
        a[5] = cmul(a[5], cmul(b4, b));
      }
      if constexpr (R > 6) {
        a[6] = cmul(a[6], cmul(b4, b2));
        a[7] = cmul(a[7], cmul(b4, cmul(b2, b)));
      }
      if constexpr (R > 8) {
        const cf b8 = cmul(b4, b4);
        a[8]        = cmul(a[8], b8);
        a[9]        = cmul(a[9], cmul(b8, b));
        a[10]       = cmul(a[10], cmul(b8, b2));
        a[11]       = cmul(a[11], cmul(b8, cmul(b2, b)));
        if constexpr (R > 12) {
          const cf b12 = cmul(b8, b4);
          a[12]        = cmul(a[12], b12);
          a[13]        = cmul(a[13], cmul(b12, b));
          a[14]        = cmul(a[14], cmul(b12, b2));
          a[15]        = cmul(a[15], cmul(b12, cmul(b2, b)));
        }
      }
    }
  }
}

// LDS index padding: one extra element every 16 keeps the stride-16 stores of the first stage off a single bank.
__device__ __forceinline__ uint32_t pad(uint32_t i)
{
  return i + (i >> 4);
}

// pad(base + k * C) for k = 0, 1, ... from pb = pad(base): where the step is a multiple of 16 elements the padding is affine in k --
// (base + k C) >> 4 = (base >> 4) + k C / 16 -- so ONE address register serves all k and the rest is the instruction's immediate
// offset.  Written as pad(base + k * C) the compiler does not see that and keeps a register per address: sixteen per stage and
// direction, alive across the whole kernel -- 64 of the modulator's 160 vector registers.
template <int C>
__device__ __forceinline__ uint32_t pad_step(uint32_t base, uint32_t pb, int k)
{
  if constexpr (C % 16 == 0) {
    return pb + (uint32_t)k * (uint32_t)(C + C / 16);
  } else {
    return pad(base + (uint32_t)k * (uint32_t)C);
  }
}

// Radix plans: N = R0 * R1 * R2 * R3 (R2 = 1 when two stages suffice, R3 = 1 when three do), T = threads per
// transform = N / 16.
struct ThreeStages {
  static constexpr int R3 = 1;
};
template <int N>
struct Plan;
template <> struct Plan<4096> : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 16, T = 256; };
template <> struct Plan<2048> : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 8, T = 128; };
template <> struct Plan<1024> : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 4, T = 64; };
template <> struct Plan<512>  : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 2, T = 64; };
template <> struct Plan<256>  : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 1, T = 64; };
template <> struct Plan<128>  : ThreeStages { static constexpr int R0 = 16, R1 = 8, R2 = 1, T = 64; };
// 3 * 2^k (the 23.04 MHz family of sampling rates): the factor 3 (x 1, 2, 4) is the last, twiddle-free stage.
template <> struct Plan<3072> : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 12, T = 256; };
template <> struct Plan<1536> : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 6, T = 128; };
template <> struct Plan<768>  : ThreeStages { static constexpr int R0 = 16, R1 = 16, R2 = 3, T = 64; };
template <> struct Plan<384>  : ThreeStages { static constexpr int R0 = 16, R1 = 8, R2 = 3, T = 64; };
// 6144 = 3 * 2^11 and 4608 = 9 * 2^9 (the next sizes of the reference's generic DFT, dft_processor_generic_impl.cpp:201-202;
// 6144 is the 15 kHz transform of a 92.16 MHz sampling rate): four stages, still one transform per workgroup in LDS
// (52 KB / 39 KB); the last, twiddle-free stage is the radix 3.
template <> struct Plan<6144> { static constexpr int R0 = 16, R1 = 16, R2 = 8, R3 = 3, T = 384; };
template <> struct Plan<4608> { static constexpr int R0 = 16, R1 = 16, R2 = 6, R3 = 3, T = 288; };

// Input index k-th element of the first-stage butterfly of thread `tid`: x[tid + k * N / R0].
template <int N>
__device__ __forceinline__ uint32_t first_stage_index(uint32_t tid, int k)
{
  return tid + k * (N / Plan<N>::R0);
}

// Twiddle bases of a thread: stage s multiplies output j of its butterfly by (w_n^p)^j with w_n^p = tw[p * S].
template <int N>
struct TwiddleBase {
  cf b0, b1, b2; // first, second and (four-stage plans) third stage; the last stage of a plan has n1 = 1: no twiddles
};

template <int SIGN, int N>
__device__ __forceinline__ TwiddleBase<N> load_twiddle_base(const float2* __restrict__ tw, uint32_t tid)
{
  using P = Plan<N>;
  TwiddleBase<N> t;
  // Stage 0: S = 1, p = butterfly index = tid (threads beyond N/R0 butterflies are idle in that stage).
  const float2 w0 = tw[tid % N];
  // Stage 1: S = R0, p = b / R0 for butterfly b = tid (+ it*T); only the first iteration's base is kept here, the
  // others are derived in the stage (see stage_lds).
  const float2 w1 = tw[((tid / P::R0) * P::R0) % N];
  t.b0            = make_cf(w0.x, SIGN < 0 ? -w0.y : w0.y);
  t.b1            = make_cf(w1.x, SIGN < 0 ? -w1.y : w1.y);
  t.b2            = t.b1;
  if constexpr (P::R3 != 1) { // stage 2: S = R0 R1
    const float2 w2 = tw[((tid / (P::R0 * P::R1)) * (P::R0 * P::R1)) % N];
    t.b2            = make_cf(w2.x, SIGN < 0 ? -w2.y : w2.y);
  }
  return t;
}

// First Stockham stage on registers a[k] = x[tid + k N/R0]: y[R0 p + j] = DFT(a)[j] * w^(j p), p = tid, S = 1.
template <int SIGN, int N>
__device__ __forceinline__ void stage_first(cf (&a)[Plan<N>::R0], cf base, cf* lds, uint32_t tid)
{
  constexpr int R  = Plan<N>::R0;
  constexpr int NB = N / R;
  if (NB >= Plan<N>::T || tid < NB) {
    Butterfly<SIGN, R>::run(a);
    apply_twiddle_powers<R>(base, a);
    const uint32_t pb = pad(R * tid);
#pragma unroll
    for (int j = 0; j != R; ++j) {
      lds[R == 16 ? pb + j : pad(R * tid + j)] = a[j]; // (R = 16: the sixteen outputs share one padding step)
    }
  }
  __syncthreads();
}

// A sink that wants the R outputs of a last-stage thread in one call says so with a member constant `all_outputs`.
// (std::is_invocable on the sink's call operator is no test for it: the trait is evaluated inside host-side library templates,
// where a __device__ operator is never viable -- it answered "no" for every sink, and until round 4 both modulator kernels
// silently took the one-output-at-a-time form.)
template <typename Store, typename = void>
struct takes_all_outputs : std::false_type {};
template <typename Store>
struct takes_all_outputs<Store, std::void_t<decltype(Store::all_outputs)>> : std::bool_constant<Store::all_outputs> {};

// A later Stockham stage (decimation in frequency, autosort).  n = N / S is the current transform length.
//   a[k] = x[q + S (p + k n/R)],   y[q + S (R p + j)] = DFT_R(a)[j] * w_n^(j p),   p < n/R, q < S.
template <int SIGN, int N, int T, int R, int S, bool LAST, typename Store>
__device__ __forceinline__ void stage_lds(cf* lds, const float2* __restrict__ tw, cf base, uint32_t tid,
                                          Store store)
{
  constexpr int NB    = N / R;
  constexpr int ITERS = (NB + T - 1) / T;
  constexpr int n1    = N / S / R;
  cf            a[ITERS][R];
#pragma unroll
  for (int it = 0; it != ITERS; ++it) {
    uint32_t b = tid + it * T;
    if (NB % T == 0 || b < NB) {
      uint32_t p = b / S, q = b % S;
      const uint32_t rb = q + S * p, prb = pad(rb);
#pragma unroll
      for (int k = 0; k != R; ++k) {
        a[it][k] = lds[pad_step<S * n1>(rb, prb, k)];
      }
    }
  }
  __syncthreads(); // every read of this stage is done before anyone overwrites
#pragma unroll
  for (int it = 0; it != ITERS; ++it) {
    uint32_t b = tid + it * T;
    if (NB % T == 0 || b < NB) {
      uint32_t p = b / S, q = b % S;
      Butterfly<SIGN, R>::run(a[it]);
      if constexpr (n1 > 1) {
        cf bs = base;
        if (it > 0) { // p differs per iteration: fetch this iteration's base (rare plans only)
          const float2 w = tw[(p * S) % N];
          bs             = make_cf(w.x, SIGN < 0 ? -w.y : w.y);
        }
        apply_twiddle_powers<R>(bs, a[it]);
      }
      if constexpr (LAST) {
        // The last stage has S * R = N, hence p = 0: output index = q + S * j, a per-thread part and a constant.
        static_assert(S * R == N, "last stage");
        if constexpr (takes_all_outputs<Store>::value) {
          store(q, Const<S>{}, a[it]); // the sink takes the thread's R outputs together (it may pair them up)
        } else {
          static_for<R>([&](auto J) { store(q, Const<S * decltype(J)::value>{}, Const<S>{}, a[it][decltype(J)::value]); });
        }
      } else {
        const uint32_t wb = q + S * R * p, pwb = pad(wb);
#pragma unroll
        for (int j = 0; j != R; ++j) {
          lds[pad_step<S>(wb, pwb, j)] = a[it][j];
        }
      }
    }
  }
  if (!LAST) {
    __syncthreads();
  }
}

template <int SIGN, int N, typename Store>
__device__ __forceinline__ void fft_from_registers(cf (&a)[Plan<N>::R0], const TwiddleBase<N>& tb, cf* lds,
                                                   const float2* __restrict__ tw, uint32_t tid, Store store)
{
  using P = Plan<N>;
  constexpr int T = P::T;
  auto no_store   = [](uint32_t, auto, auto, cf) {};
  stage_first<SIGN, N>(a, tb.b0, lds, tid);
  if constexpr (P::R2 == 1) {
    stage_lds<SIGN, N, T, P::R1, P::R0, true>(lds, tw, tb.b1, tid, store);
  } else if constexpr (P::R3 == 1) {
    stage_lds<SIGN, N, T, P::R1, P::R0, false>(lds, tw, tb.b1, tid, no_store);
    stage_lds<SIGN, N, T, P::R2, P::R0 * P::R1, true>(lds, tw, tb.b1, tid, store);
  } else {
    stage_lds<SIGN, N, T, P::R1, P::R0, false>(lds, tw, tb.b1, tid, no_store);
    stage_lds<SIGN, N, T, P::R2, P::R0 * P::R1, false>(lds, tw, tb.b2, tid, no_store);
    stage_lds<SIGN, N, T, P::R3, P::R0 * P::R1 * P::R2, true>(lds, tw, tb.b2, tid, store);
  }
  __syncthreads(); // the LDS buffer is reused by the next transform of this workgroup
}

} // namespace nrphy
