// Open Fronthaul uplink receive for gfx950 (MI355X): user-plane PRB records in device memory to the receive grid, to a
// row of cbf16 and to the PRACH buffer.  One decompression core (ofh_ul_chunk, ofh_ul_chunk_device.h: ofh_rx_kernels.hip shares
// it), three sinks.
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
#include "ofh_ul_chunk_device.h"

namespace nrphy {

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
