// Open Fronthaul uplink receive for gfx950 (MI355X): user-plane PRB records in device memory to the receive grid, to a
// row of cbf16 and to the PRACH buffer.  One decompression core, three sinks.
//
//   ofh_ul_rows_kernel      nrphy_ofh_decompress: rows of records to rows of cbf16 (iq_decompressor::decompress)
//   ofh_ul_sections_kernel  nrphy_ofh_ul_write_grid / nrphy_ofh_ul_write_prach: a host-built list of items, each a run
//                           of records and the resource elements of it that go to a destination
//                           (uplane_rx_symbol_data_flow_writer::write_to_resource_grid,
//                           uplane_prach_symbol_data_flow_writer::write_to_prach_buffer)
//
// Arithmetic: R/lib/ofh/compression/iq_compression_none_impl.cpp:56-73, iq_compression_bfp_impl.cpp:98-135, quantizer.h,
// compressed_prb_unpacker.cpp, R/include/srsran/adt/bf16.h:39-56.
//
// The kernels are memory bound (3 w (+ 1) bytes in, 48 or 96 out per PRB).  A workgroup is one wave and takes
// OFH_UL_PRBS_PER_WG consecutive records of one item.  They are contiguous and byte-aligned, so the wave copies their span
// into LDS with aligned dword loads -- the dwords that the span covers only in part, its first and its last, go byte by
// byte, so that nothing outside the span is read -- and unpacks from LDS.  Lane l then owns resource elements l, l + 64 and
// l + 128 of the 192 of the chunk: consecutive lanes store consecutive 4-byte (cbf16) or 8-byte (complex float) words.
#include "bits_device.h"

namespace nrphy {

constexpr uint32_t OFH_UL_MAX_RECORD = 49; // 3 * 16 + 1
static_assert(OFH_UL_PRBS_PER_WG * 12 == 3 * WAVE, "three resource elements per lane");
// dwords that a chunk's span can touch (it starts at byte 0..3 of the first), in passes of one dword per lane
constexpr uint32_t OFH_UL_STAGE_PASSES = ((OFH_UL_PRBS_PER_WG * OFH_UL_MAX_RECORD + 3 + 3) / 4 + WAVE - 1) / WAVE;

// Records first_prb ... of the item that starts at `src`, `count` of them, to the resource elements of the item's range
// [re_skip, re_skip + nof_re) that fall into them; element re_skip goes to dst[0].  Every lane of the wave comes here.
template <bool PRACH>
__device__ __forceinline__ void ofh_ul_chunk(const uint8_t* __restrict__ src, uint32_t first_prb, uint32_t count, uint32_t re_skip,
                                             uint32_t nof_re, uint32_t w, uint32_t bfp, void* __restrict__ dst)
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
    if (local < 12u * count && re >= re_skip && re - re_skip < nof_re) {
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

__global__ __launch_bounds__(WAVE) void ofh_ul_rows_kernel(OfhDecompressLaunch p)
{
  const uint32_t first = blockIdx.x * OFH_UL_PRBS_PER_WG, row = blockIdx.y;
  const uint32_t count = first < p.nof_prb ? min(OFH_UL_PRBS_PER_WG, p.nof_prb - first) : 0u;
  ofh_ul_chunk<false>(p.in + (size_t)row * p.in_row_stride, first, count, 0u, 12u * p.nof_prb, p.data_width, p.bfp,
                      p.prbs + (size_t)row * p.row_stride);
}

template <bool PRACH>
__global__ __launch_bounds__(WAVE) void ofh_ul_sections_kernel(const OfhUlItem* __restrict__ items, uint32_t n, const uint8_t* __restrict__ payload,
                                                               void* __restrict__ dst)
{
  // The item whose chunks include this workgroup's: the last one with first_chunk <= blockIdx.x (wave-uniform).
  const NRPHY_CONSTANT OfhUlItem* it = to_constant(items);
  uint32_t                        lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (it[mid].first_chunk <= blockIdx.x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const uint32_t re_skip = it[lo].re_skip, nof_re = it[lo].nof_re;
  const uint32_t nof_prb = (re_skip + nof_re + 11u) / 12u, first = (blockIdx.x - it[lo].first_chunk) * OFH_UL_PRBS_PER_WG;
  const uint32_t count   = first < nof_prb ? min(OFH_UL_PRBS_PER_WG, nof_prb - first) : 0u;
  uint8_t*       dst_item = reinterpret_cast<uint8_t*>(dst) + it[lo].dst * (PRACH ? 8u : 4u);
  ofh_ul_chunk<PRACH>(payload + it[lo].src, first, count, re_skip, nof_re, it[lo].data_width, it[lo].bfp, dst_item);
}

hipError_t launch_ofh_decompress(const OfhDecompressLaunch& p, uint32_t n_rows, hipStream_t stream)
{
  if (n_rows == 0 || p.nof_prb == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ofh_ul_rows_kernel, dim3((p.nof_prb + OFH_UL_PRBS_PER_WG - 1) / OFH_UL_PRBS_PER_WG, n_rows), dim3(WAVE), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_ofh_ul_sections(const OfhUlItem* d_items, uint32_t n, uint32_t nof_chunks, const uint8_t* d_payload, void* d_dst,
                                  bool prach, hipStream_t stream)
{
  if (n == 0 || nof_chunks == 0) {
    return hipSuccess;
  }
  if (prach) {
    hipLaunchKernelGGL(ofh_ul_sections_kernel<true>, dim3(nof_chunks), dim3(WAVE), 0, stream, d_items, n, d_payload, d_dst);
  } else {
    hipLaunchKernelGGL(ofh_ul_sections_kernel<false>, dim3(nof_chunks), dim3(WAVE), 0, stream, d_items, n, d_payload, d_dst);
  }
  return hipGetLastError();
}

} // namespace nrphy
