// Open Fronthaul downlink transmit for gfx950 (MI355X): OFDM symbols of the device-resident downlink grid to complete
// Ethernet frames -- VLAN Ethernet, eCPRI, radio-application and section headers, compressed PRB records, padding -- in one
// launch for a batch of (slot, eAxC, symbol) descriptors.
//
//   ofh_dl_frames_kernel   nrphy_ofh_dl_write_frames / nrphy_ofh_dl_frames_host
//                          (data_flow_uplane_downlink_data_impl::enqueue_section_type_1_message:
//                          R/lib/ofh/transmitter/ofh_data_flow_uplane_downlink_data_impl.cpp:104-215,
//                          ofh_uplane_fragment_size_calculator.cpp, R/lib/ofh/ethernet/vlan_ethernet_frame_builder_impl.cpp,
//                          R/lib/ofh/ecpri/ecpri_packet_builder_impl.cpp, R/lib/ofh/serdes/ofh_uplane_message_builder_impl.cpp
//                          and its _static_/_dynamic_compression_impl.cpp, R/include/srsran/ofh/ethernet/ethernet_frame_pool.h:63-71)
//
// A fragment of a symbol is one frame and one compress() call of the reference: the records come from ofh_compress_prb with
// the PRB's number inside the fragment and the fragment's PRB count, which is what decides where the reference's vector loop
// ends and its rounding changes.
//
// The kernel is memory bound (48 B in, 3 w (+ 1) B out per PRB).  The records start 34 or 36 bytes into a frame and are
// 3 w (+ 1) bytes long, so neither they nor any fixed number of them line up with the frame's dwords.  The work is therefore
// cut by bytes of the frame, not by PRBs: a workgroup (one wave) owns one window of the frame that starts and ends on 16-byte
// boundaries of the frame's address (the first window starts with the frame, the last ends with it).  It compresses every
// PRB that has a byte in the window -- one lane per PRB, three 16-byte loads of the PRB's 12 cbf16 -- into LDS at the
// position the byte has in the window, the first window adds the header and the padding, and then consecutive lanes store
// consecutive aligned 16-byte blocks.  A PRB on a window's edge is compressed by both neighbours (at most 2 of ~62 PRBs
// of a window); in exchange only the head of a frame whose address is not 16-byte aligned and the last 15 bytes of a frame
// go out as dword or byte stores.  Nothing outside the frame's frame_bytes bytes is written.
#include "ofh_compress_device.h"

namespace nrphy {

// A window is at most 62 records long, so at most 64 records have a byte in it.
constexpr uint32_t OFH_DL_LDS_BYTES = 16 + 64 * OFH_MAX_RECORD + 64;

__global__ __launch_bounds__(WAVE) void ofh_dl_frames_kernel(const OfhDlSymbol* __restrict__ symbols, uint32_t n, const uint32_t* __restrict__ grid,
                                                             uint8_t* __restrict__ frames)
{
  __shared__ __attribute__((aligned(16))) uint8_t s_out[OFH_DL_LDS_BYTES];
  // The descriptor whose workgroups include this one: the last with first_wg <= blockIdx.x (wave-uniform).
  const NRPHY_CONSTANT OfhDlSymbol* it = to_constant(symbols);
  uint32_t                          lo = 0, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (it[mid].first_wg <= blockIdx.x) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const NRPHY_CONSTANT OfhDlSymbol& d = it[lo];
  const uint32_t lane = threadIdx.x, wg = blockIdx.x - d.first_wg;
  const uint32_t nof_frags = d.nof_frags, ppf = d.prbs_per_frag, w = d.data_width, bfp = d.bfp, hdr = d.header_bytes;
  const uint32_t rec = 3u * w + bfp;
  const uint32_t frag = min(wg / d.windows_per_frag, nof_frags - 1u), win = wg - frag * d.windows_per_frag;
  const uint32_t start_prb = frag * ppf, frag_prbs = min(ppf, (uint32_t)d.nof_prbs - start_prb);
  const uint32_t used = hdr + frag_prbs * rec, frame_bytes = max(used, 64u);
  uint8_t*       frame = frames + d.frame + (uint64_t)frag * d.stride;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(frame) & 15u);
  // The window in bytes of the frame, [wlo, whi): 16-byte boundaries of the address, clamped to the frame.
  const uint32_t wlo = win == 0 ? 0u : win * d.window - mis, whi = min(frame_bytes, (win + 1u) * d.window - mis);
  if (wlo >= whi) {
    return;
  }
  // The records with a byte in the window, [p_lo, p_hi) of the fragment.
  const uint32_t p_lo = wlo <= hdr ? 0u : (wlo - hdr) / rec;
  const uint32_t p_hi = whi <= hdr ? 0u : min(frag_prbs, (whi - hdr + rec - 1u) / rec);
  // LDS byte i holds frame byte base + i; base is a 16-byte boundary of the address at or below everything staged
  // (negative for the first window of a frame whose address is not aligned).
  const int32_t first_staged = (int32_t)(p_lo < p_hi ? min(wlo, hdr + p_lo * rec) : wlo);
  const int32_t base         = (int32_t)((((uint32_t)first_staged + mis) & ~15u)) - (int32_t)mis;

  if (lane < p_hi - p_lo && p_lo < p_hi) {
    const uint32_t prb = p_lo + lane; // in the fragment = in the reference's compress() call
    uint32_t       in[12];
    if (start_prb + prb < d.grid_prbs) {
      const uint4* src = reinterpret_cast<const uint4*>(grid + d.row + 12u * (start_prb + prb));
#pragma unroll
      for (uint32_t k = 0; k != 3; ++k) {
        const uint4 v = src[k];
        in[4 * k] = v.x, in[4 * k + 1] = v.y, in[4 * k + 2] = v.z, in[4 * k + 3] = v.w;
      }
    } else {
#pragma unroll
      for (uint32_t k = 0; k != 12; ++k) {
        in[k] = 0u; // the reference's zero-filled temporary buffer
      }
    }
    ofh_compress_prb(in, prb, frag_prbs, w, bfp, d.whole_span, d.scale, s_out + ((int32_t)(hdr + prb * rec) - base));
  }
  if (win == 0) {
    // Header of this fragment, and zeros up to 64 bytes (frame_buffer::set_size).
    if (lane < hdr) {
      const uint32_t size = used - 22u; // eCPRI payload: everything after its 4-byte common header
      uint32_t       b    = d.header[lane];
      b                   = lane == 20u ? size >> 8 : b;
      b                   = lane == 21u ? size & 0xFFu : b;
      b                   = lane == 24u ? b + frag : b;  // sequence identifier, modulo 256
      b                   = lane == 31u ? (start_prb >> 8) & 3u : b; // every RB, this symbol, 2 MSBs of startPrbu
      b                   = lane == 32u ? start_prb & 0xFFu : b;
      b                   = lane == 33u ? (frag_prbs > 255u ? 0u : frag_prbs) : b;
      s_out[(int32_t)lane - base] = (uint8_t)b;
    }
    if (used + lane < frame_bytes) {
      s_out[(int32_t)(used + lane) - base] = 0;
    }
  }
  __syncthreads();
  // 16-byte blocks of LDS that the window touches; all but the frame's head and tail lie inside it.
  const uint32_t b_first = (uint32_t)((int32_t)wlo - base) >> 4, b_last = ((uint32_t)((int32_t)whi - base) + 15u) >> 4;
  for (uint32_t b = b_first + lane; b < b_last; b += WAVE) {
    const int32_t at = base + (int32_t)(16u * b); // frame byte of the block's first byte
    if (at >= (int32_t)wlo && at + 16 <= (int32_t)whi) {
      *reinterpret_cast<uint4*>(frame + at) = *reinterpret_cast<const uint4*>(s_out + 16u * b);
    } else {
      for (uint32_t q = 0; q != 4; ++q) {
        const int32_t a4 = at + (int32_t)(4u * q);
        if (a4 >= (int32_t)wlo && a4 + 4 <= (int32_t)whi) {
          *reinterpret_cast<uint32_t*>(frame + a4) = *reinterpret_cast<const uint32_t*>(s_out + 16u * b + 4u * q);
        } else {
          for (int32_t a = a4; a != a4 + 4; ++a) {
            if (a >= (int32_t)wlo && a < (int32_t)whi) {
              frame[a] = s_out[a - base];
            }
          }
        }
      }
    }
  }
}

hipError_t launch_ofh_dl_frames(const OfhDlSymbol* d_symbols, uint32_t n, uint32_t nof_wgs, const uint32_t* d_grid, uint8_t* d_frames,
                                hipStream_t stream)
{
  if (n == 0 || nof_wgs == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ofh_dl_frames_kernel, dim3(nof_wgs), dim3(WAVE), 0, stream, d_symbols, n, d_grid, d_frames);
  return hipGetLastError();
}

} // namespace nrphy
