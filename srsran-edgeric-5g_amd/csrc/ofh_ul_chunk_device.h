// The decompression core of the Open Fronthaul uplink receive, shared by ofh_ul_kernels.hip (rows of records, host-built
// section lists) and ofh_rx_kernels.hip (whole Ethernet frames): one wave takes OFH_UL_PRBS_PER_WG consecutive records, stages
// their bytes in LDS and stores three resource elements per lane.
#pragma once
#include "bits_device.h"

namespace nrphy {

// Which PRBs of an item a wave may store: all of them, for the callers whose destinations are disjoint by validation.
struct OfhUlKeepAll {
  __device__ __forceinline__ bool operator()(uint32_t) const { return true; }
};

constexpr uint32_t OFH_UL_MAX_RECORD = 49; // 3 * 16 + 1
static_assert(OFH_UL_PRBS_PER_WG * 12 == 3 * WAVE, "three resource elements per lane");
// dwords that a chunk's span can touch (it starts at byte 0..3 of the first), in passes of one dword per lane
constexpr uint32_t OFH_UL_STAGE_PASSES = ((OFH_UL_PRBS_PER_WG * OFH_UL_MAX_RECORD + 3 + 3) / 4 + WAVE - 1) / WAVE;

// Records first_prb ... of the item that starts at `src`, `count` of them, to the resource elements of the item's range
// [re_skip, re_skip + nof_re) that fall into them; element re_skip goes to dst[0].  Every lane of the wave comes here.
// keep(prb) says whether record `prb` of the item is stored at all (the frame receiver's "later message wins").
template <bool PRACH, typename Keep = OfhUlKeepAll>
__device__ __forceinline__ void ofh_ul_chunk(const uint8_t* __restrict__ src, uint32_t first_prb, uint32_t count, uint32_t re_skip,
                                             uint32_t nof_re, uint32_t w, uint32_t bfp, void* __restrict__ dst, Keep keep = Keep())
{
  // + 4: the span sits at its address modulo 4; + 8: the 5 bytes an unpack reads may end past the last record
  __shared__ __attribute__((aligned(4))) uint8_t s_in[OFH_UL_PRBS_PER_WG * OFH_UL_MAX_RECORD + 4 + 8];
  const uint32_t lane = threadIdx.x, rec = 3u * w + bfp;
  const uint8_t* p    = src + (size_t)first_prb * rec;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u), end = mis + count * rec;
  const uint8_t* base = p - mis; // 4-byte aligned; only bytes [mis, end) of it are read
  // All of the wave's dword loads are issued before the first is stored: one round trip to memory, not one per pass.
  uint32_t staged[OFH_UL_STAGE_PASSES];
#pragma unroll
  for (uint32_t k = 0; k != OFH_UL_STAGE_PASSES; ++k) {
    const uint32_t d = lane + WAVE * k, lo = 4u * d;
    staged[k]        = (lo >= mis && lo + 4u <= end) ? reinterpret_cast<const uint32_t*>(base)[d] : 0u;
  }
#pragma unroll
  for (uint32_t k = 0; k != OFH_UL_STAGE_PASSES; ++k) {
    const uint32_t d = lane + WAVE * k, lo = 4u * d;
    if (lo >= mis && lo + 4u <= end) {
      reinterpret_cast<uint32_t*>(s_in)[d] = staged[k];
    } else if (lo < end) {
      for (uint32_t b = lo; b != lo + 4u; ++b) {
        if (b >= mis && b < end) {
          s_in[b] = base[b];
        }
      }
    }
  }
  __syncthreads();
  const float gain = bfp ? 32767.0f : (float)((1 << (w - 1u)) - 1);
#pragma unroll
  for (uint32_t j = 0; j != 3; ++j) {
    const uint32_t local = lane + WAVE * j, re = 12u * first_prb + local;
    if (local < 12u * count && re >= re_skip && re - re_skip < nof_re && keep(first_prb + local / 12u)) {
      const uint8_t* r      = s_in + mis + (local / 12u) * rec;
      const uint32_t bitpos = 8u * bfp + 2u * w * (local % 12u), sh = bitpos & 7u, need = (sh + 2u * w + 7u) >> 3;
      const uint8_t* q      = r + (bitpos >> 3);
      uint64_t       acc    = 0;
#pragma unroll
      for (uint32_t b = 0; b != 5; ++b) {
        acc = (acc << 8) | (b < need ? (uint64_t)q[b] : 0u);
      }
      // compressed_prb_unpacker::unpack + quantizer::sign_extend: data_width bits, most significant first, as int16
      const uint32_t fi = (uint32_t)(acc >> (40u - sh - w)), fq = (uint32_t)(acc >> (40u - sh - 2u * w));
      int            vi = (int)(fi << (32u - w)) >> (32u - w), vq = (int)(fq << (32u - w)) >> (32u - w);
      if (bfp) {
        // int16_t scaler = 1 << udCompParam as the reference's compiler evaluates it: 2^e, -32768 for e = 15, 0 above
        const uint32_t e      = r[0];
        const int      scaler = e <= 15u ? (int)(int16_t)(uint16_t)(1u << e) : 0;
        vi *= scaler;
        vq *= scaler;
      }
      // quantizer::to_float: int -> float, then a correctly rounded division (never a reciprocal multiplication)
      const uint32_t bi = to_bf16_bits(__fdiv_rn((float)vi, gain)), bq = to_bf16_bits(__fdiv_rn((float)vq, gain));
      if (PRACH) {
        // srsvec::convert(cf, cbf16): each half widened
        reinterpret_cast<float2*>(dst)[re - re_skip] = make_float2(__uint_as_float(bi << 16), __uint_as_float(bq << 16));
      } else {
        reinterpret_cast<uint32_t*>(dst)[re - re_skip] = bi | (bq << 16);
      }
    }
  }
}


} // namespace nrphy
