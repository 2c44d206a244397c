// The low-PAPR base sequences r_{u,0}(n) of TS 38.211 Section 5.2.2 as low_papr_sequence_generator_impl::generate(u, 0, 0, 1)
// produces them (R/lib/phy/upper/sequence_generators/low_papr_sequence_generator_impl.cpp:158-244): every element is an entry
// of a complex_exponential_table, and what is defined here, once, is the entry's index.  The element itself is
// unit_circle(index, size) of exact_device.h for the SRS estimator, whose recorded answers are met within their tolerance and
// whose bytes stay what they were, and unit_circle_libm(index, size) below for the PUSCH DM-RS, which is pinned to the recorded
// sequences bit for bit.  Included by the SRS estimator (srs_kernels.hip) and by the PUSCH DM-RS estimator
// (pusch_chest_kernels.hip); the root q of the Zadoff-Chu sizes is evaluated on the host (low_papr_host.h).
#pragma once

#include "exact_device.h"

namespace nrphy {

constexpr uint32_t LOW_PAPR_TABLE_CIRCLE = 8;  // M_zc = 6, 12, 18, 24: exp(j phi pi / 4)
constexpr uint32_t LOW_PAPR_ZC30_CIRCLE  = 62; // M_zc = 30: exp(-j pi (u + 1)(n + 1)(n + 2) / 31)

// complex_exponential_table(size, 1)[index] with the bits the reference's build gives it: std::polar(1.0F, x), x =
// float(2 pi) float(index) / float(size), is cosf and sinf of the C library, and those are not correctly rounded -- 1.3 % of the
// entries of the tables a PUSCH DM-RS needs are one float32 step from cos and sin evaluated in double and rounded once, which is
// what unit_circle() gives (and the SRS estimator keeps).  The library's single-precision sine and cosine (glibc 2.28 and later,
// from the Arm Optimized Routines: sincosf.h) are a quadrant reduction and two polynomials in double, rounded once to float;
// restated here operation by operation, for 0 <= x < 120, contraction off.  tests/pusch_lowpapr_model.py has the same in NumPy
// and is checked against the recorded tables.
__device__ __forceinline__ float2 unit_circle_libm(uint32_t index, uint32_t size)
{
  constexpr double HPI_INV = 0x1.45F306DC9C883p+23, HPI = 0x1.921FB54442D18p0; // 2^24 x 2 / pi, pi / 2
  constexpr double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                   C4 = 0x1.99343027bf8c3p-16;
  constexpr double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
  const float y = __fdiv_rn(__fmul_rn(TWOPI_F, (float)index), (float)size);
  if (y < 0x1p-12f) {
    return make_float2(1.f, y);
  }
  double  x = (double)y;
  int32_t n = 0;
  if (!(y < 0.75f)) { // (the library compares the top 12 bits with those of pi / 4)
    n = ((int32_t)(x * HPI_INV) + 0x800000) >> 24;
    x = x - (double)n * HPI;
  }
  const double x2 = x * x;
  const double xs = ((n + 1) & 2) ? -x : x;      // the sine's sign in quadrants 1 and 2
  const double x3 = x2 * xs, x4 = x2 * x2;
  const double c2 = C3 + x2 * C4, s1 = S2 + x2 * S3, c1 = C0 + x2 * C1;
  const double x5 = x3 * x2, x6 = x4 * x2;
  const double s = xs + x3 * S1, c = c1 + x4 * C2;
  const float  sv = (float)(s + x5 * s1);
  float        cv = (float)(c + x6 * c2);
  cv              = (n & 2) ? -cv : cv;          // quadrants 2 and 3: the cosine polynomial's coefficients negated
  return (n & 1) ? make_float2(sv, cv) : make_float2(cv, sv); // odd quadrants: the two swap
}

// M_zc = 6, 12, 18, 24: entry (8 + phi) mod 8 of the 8-point circle, phi in {-3, -1, 1, 3}.
__device__ __forceinline__ uint32_t low_papr_table_index(int phi)
{
  return (uint32_t)(8 + phi) & 7u;
}

// M_zc >= 36, Zadoff-Chu: entry (2 N_zc - (q m (m + 1) mod 2 N_zc)) mod 2 N_zc of the 2 N_zc-point circle, m = n mod N_zc.  The
// product needs 64 bits: 1619 x 1619 x 1620 at 270 PRB.
__device__ __forceinline__ uint32_t low_papr_zc_index(uint32_t q, uint32_t n_zc, uint32_t n)
{
  const uint32_t size = 2u * n_zc;
  const uint64_t m    = n % n_zc;
  const uint32_t arg  = (uint32_t)(((uint64_t)q * m * (m + 1u)) % size);
  return arg == 0u ? 0u : size - arg;
}

// M_zc = 30 (TS 38.211 Section 5.2.2.1; the reference's generator has no such size): entry
// (62 - ((u + 1)(n + 1)(n + 2) mod 62)) mod 62 of the 62-point circle.
__device__ __forceinline__ uint32_t low_papr_zc30_index(uint32_t u, uint32_t n)
{
  const uint32_t arg = ((u + 1u) * (n + 1u) * (n + 2u)) % LOW_PAPR_ZC30_CIRCLE;
  return arg == 0u ? 0u : LOW_PAPR_ZC30_CIRCLE - arg;
}

} // namespace nrphy
