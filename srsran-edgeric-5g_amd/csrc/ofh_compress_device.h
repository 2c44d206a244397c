// Open Fronthaul compression of one PRB, shared by ofh_compress_kernel (lower_phy_kernels.hip: rows of records) and
// ofh_dl_frames_kernel (ofh_dl_kernels.hip: whole Ethernet frames): 16-bit quantisation, block floating point exponent, bit
// packing (R/lib/ofh/compression/iq_compression_{none,bfp}_impl.cpp, quantizer.h, compressed_prb_packer.cpp,
// R/lib/ofh/serdes/ofh_uplane_message_builder_impl.cpp:137-144).
#pragma once
#include "bits_device.h"

namespace nrphy {

constexpr uint32_t OFH_MAX_RECORD = 49; // 3 * 16 + 1

// One value through the reference's conversion: its 16-lane vector loop rounds to nearest even and saturates
// (_mm256_cvtps_epi32 + _mm256_packs_epi32), the scalar tail of a call rounds half away from zero (std::round).
__device__ __forceinline__ int to_int16_ref(float v, bool vector_lane)
{
  if (vector_lane) {
    const int r = __float2int_rn(v);
    return r > 32767 ? 32767 : (r < -32768 ? -32768 : r);
  }
  return (int)(int16_t)(int)roundf(v);
}

// PRB number `prb` of a compress() call of `nof_prb` PRBs: the 12 cbf16 words `in` to its record at `o`
// (3 * w bytes, one more in front for BFP).
__device__ __forceinline__ void ofh_compress_prb(const uint32_t (&in)[12], uint32_t prb, uint32_t nof_prb, uint32_t w, uint32_t bfp,
                                                 uint32_t whole_span, float scale, uint8_t* o)
{
  int q[24];
  // Quantisation (quantizer::to_fixed_point through srsvec::convert, conversion.cpp:202-230): value * scale to int16.
  // The reference's AVX2 compressors convert all PRBs of a call in one go (the first 16 * floor(24 n / 16) values in
  // the vector loop) except for the widths their packer lacks, which go PRB by PRB (16 of 24 in the vector loop).
  const uint32_t n_vec = whole_span ? ((24u * nof_prb) / 16u) * 16u : 0u;
  int            vmax = -32768, vmin = 32767;
#pragma unroll
  for (uint32_t k = 0; k != 12; ++k) {
    const uint32_t word = in[k];
    const float    re = __uint_as_float(word << 16), im = __uint_as_float(word & 0xFFFF0000u);
    const uint32_t i = 2u * k;
    const bool     v0 = whole_span ? 24u * prb + i < n_vec : i < 16u, v1 = whole_span ? 24u * prb + i + 1u < n_vec : i + 1u < 16u;
    q[i]              = to_int16_ref(__fmul_rn(re, scale), v0);
    q[i + 1]          = to_int16_ref(__fmul_rn(im, scale), v1);
    vmax              = max(vmax, max(q[i], q[i + 1]));
    vmin              = min(vmin, min(q[i], q[i + 1]));
  }
  uint32_t exponent = 0;
  if (bfp) {
    // Block floating point (O-RAN.WG4.CUS Annex A.1.2; iq_compression_bfp_impl.cpp:50-75, .h:63-77): the exponent
    // that makes the largest magnitude of the PRB fit data_width bits, then an arithmetic shift.
    const int      a = abs(vmax), b = abs(vmin) - 1;
    const uint32_t max_abs = (uint32_t)(a > b ? a : b) & 0xFFFFu, max_shift = 16u - w;
    uint32_t       lz = max_shift;
    if (max_abs != 0 && max_shift != 0) {
      lz = (uint32_t)__clz((int)max_abs) - 17u;
    }
    const uint32_t raw = max_shift < lz ? max_shift : lz;
    exponent           = max_shift - raw;
    *o++               = (uint8_t)exponent;
  }
  // compressed_prb_packer::pack: data_width bits per value, most significant bit first.
  uint64_t       acc = 0;
  uint32_t       nbits = 0;
  const uint32_t mask = (1u << w) - 1u;
#pragma unroll
  for (uint32_t i = 0; i != 24; ++i) {
    acc = (acc << w) | (uint64_t)((uint32_t)(q[i] >> exponent) & mask);
    nbits += w;
    while (nbits >= 8u) {
      *o++ = (uint8_t)(acc >> (nbits - 8u));
      nbits -= 8u;
    }
  }
}

} // namespace nrphy
