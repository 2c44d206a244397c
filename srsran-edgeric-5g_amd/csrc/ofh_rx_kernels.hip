// Open Fronthaul uplink frame receiver for gfx950 (MI355X): received Ethernet frames in device memory to the receive grid.
// Three launches, no host step between them:
//
//   ofh_rx_parse_kernel     one thread per frame: the Ethernet, eCPRI and user-plane headers, the section loop, the look-up of
//                           what the control plane announced and every stateless drop rule, in the reference's order
//                           (message_receiver_impl::process_new_frame and what it calls).  Byte-wise, big-endian, at any
//                           alignment; no byte at or beyond offset + length is read.  Writes the provisional record.
//   ofh_rx_sequence_kernel  one workgroup: lane k walks the frames of eAxC k in batch order through
//                           sequence_id_checker_impl::update_and_compare_seq_id (serial by nature), from one word per frame
//                           staged in LDS, which turns frames from the past into status 7; after the barrier the accepted
//                           frames claim their PRBs in the ownership table with atomicMax(frame index + 1), also from LDS:
//                           the later message wins.
//   ofh_rx_write_kernel     one wave per (frame, OFH_UL_PRBS_PER_WG PRBs): ofh_ul_chunk, the decompression core of
//                           ofh_ul_kernels.hip, storing only the PRBs whose ownership word names this frame.  Waves of frames
//                           that are not accepted, or beyond nof_prbs_written, leave at once (wave-uniform: the record is read
//                           through the scalar cache).  Memory bound like its sibling.
#include "ofh_ul_chunk_device.h"

namespace nrphy {

namespace {

__device__ __forceinline__ uint32_t be16(const uint8_t* p)
{
  return (uint32_t)p[0] << 8 | p[1];
}

__device__ __forceinline__ bool in_list(const uint16_t* list, uint32_t n, uint32_t v)
{
  bool found = false;
  for (uint32_t k = 0; k != 4; ++k) {
    found = found || (k < n && list[k] == v);
  }
  return found;
}

// Bytes of one PRB record of a section: is_ud_comp_param_present adds the udCompParam byte.
__device__ __forceinline__ uint32_t record_bytes(uint32_t type, uint32_t width)
{
  return 3u * width + ((type == 1u || type == 2u || type == 3u || type == 5u || type == 6u) ? 1u : 0u);
}

// The frame's way through the reference's receiver up to the sequence checker and past it as if the checker answered 0.
// Returns the status; fills the fields of `r` that the status says were reached.
__device__ uint32_t ofh_rx_parse(const OfhRxLaunch& p, uint64_t offset, uint32_t length, nrphy_ofh_rx_record_t& r)
{
  const uint8_t* f = p.d_frames + offset;
  // vlan_frame_decoder_impl::decode, should_ethernet_frame_be_filtered
  if (length < 64u) {
    return 1;
  }
  bool same = true;
  for (uint32_t k = 0; k != 12; ++k) {
    same = same && f[k] == p.mac[k];
  }
  uint32_t at = p.eth_header; // 14 or 18: at + 8 <= 64 <= length
  if (!same || be16(f + at - 2) != p.eth_type) {
    return 2;
  }
  // ecpri::packet_decoder_impl::decode_header, decode_payload of either decoder, should_ecpri_packet_be_filtered
  if ((f[at] >> 4) != 1u || (f[at] & 1u) != 0) {
    return 3;
  }
  const uint32_t msg_type = f[at + 1], size = be16(f + at + 2);
  at += 4;
  const uint32_t rem = length - at;
  if (!p.ignore_size && (size > rem || size < 5u)) {
    return 4;
  }
  if (msg_type != 0) {
    return 5;
  }
  const uint32_t eaxc = be16(f + at), seq_id = be16(f + at + 2);
  at += 4;
  const uint32_t msg_len = (p.ignore_size ? rem : size) - 4u; // at + msg_len <= length
  r.eaxc   = (uint16_t)eaxc;
  r.seq_id = (uint16_t)seq_id;
  if (!in_list(p.ul_eaxc, p.n_ul_eaxc, eaxc) && !in_list(p.prach_eaxc, p.n_prach_eaxc, eaxc)) {
    return 6;
  }
  // ---- the sequence checker sees the frame here (ofh_rx_sequence_kernel) ----
  // uplane_peeker::peek_slot_symbol_point, peek_filter_index
  if (msg_len < 4u) {
    return 8;
  }
  const uint8_t* m       = f + at;
  const uint32_t b0      = m[0], subframe = m[2] >> 4, slot = (uint32_t)(m[2] & 0x0Fu) << 2 | m[3] >> 6, symbol = m[3] & 0x3Fu;
  const uint32_t filter = b0 & 0x0Fu;
  if (subframe >= 10u || slot >= (1u << p.numerology)) {
    return 8;
  }
  r.sfn8         = m[1];
  r.subframe     = (uint8_t)subframe;
  r.slot         = (uint8_t)slot;
  r.symbol       = (uint8_t)symbol;
  r.filter_index = (uint8_t)filter;
  if (filter >= 8u) {
    return 9;
  }
  // uplane_message_decoder_impl::decode_header
  if ((b0 >> 7) != 0) {
    return 10;
  }
  if (((b0 >> 4) & 7u) != 1u) {
    return 11;
  }
  if (symbol >= p.nof_symbols) {
    return 12;
  }
  // decode_all_sections: an incomplete section ends the loop, a second complete one drops the message
  const uint32_t route = filter != 0 ? 1u : 0u;
  uint32_t       q = 4, nof_sections = 0, rb = 0, sym_inc = 0, start_prb = 0, nof_prbs = 0, type = 0, width = 0, records_at = 0;
  while (q < msg_len) {
    if (msg_len - q < 4u) {
      break;
    }
    const uint32_t s1 = m[q + 1];
    uint32_t       start = (s1 & 3u) << 8 | m[q + 2], n = m[q + 3];
    if (n == 0) {
      n     = p.ru_nof_prbs;
      start = 0;
    }
    q += 4;
    uint32_t t = p.type[route], w = p.data_width[route];
    if (!p.static_compression) {
      if (msg_len - q < 2u) {
        break;
      }
      t = m[q] & 0x0Fu;
      if (t >= 7u) {
        return 13;
      }
      w = m[q] >> 4;
      w = w == 0 ? 16u : w;
      q += 2;
    }
    if (t == 5u || t == 6u) { // decode_compression_length: udCompLen of the selective types
      if (msg_len - q < 2u) {
        break;
      }
      q += 2;
    }
    const uint32_t bytes = record_bytes(t, w) * n;
    if (msg_len - q < bytes) {
      break;
    }
    if (nof_sections == 0) {
      rb = (s1 >> 3) & 1u, sym_inc = (s1 >> 2) & 1u, start_prb = start, nof_prbs = n, type = t, width = w, records_at = q;
    }
    q += bytes;
    if (++nof_sections == 2u) {
      return 14;
    }
  }
  if (nof_sections == 0) {
    return 15;
  }
  r.start_prb      = (uint16_t)start_prb;
  r.nof_prbs       = (uint16_t)nof_prbs;
  r.type           = (uint8_t)type;
  r.data_width     = (uint8_t)width;
  r.payload_offset = offset + at + records_at;
  if (type > 1u || (type == 0 && width < 2u)) {
    return 16;
  }
  if (route != 0) {
    return 22;
  }
  // data_flow_uplane_uplink_data_impl::should_uplane_packet_be_filtered
  const NRPHY_CONSTANT nrphy_ofh_rx_expect_t* e = to_constant(p.expects);
  uint32_t                                    found = p.n_expect;
  for (uint32_t k = 0; k != p.n_expect; ++k) {
    if (e[k].sfn8 == r.sfn8 && e[k].subframe == subframe && e[k].slot == slot && e[k].eaxc == eaxc) {
      found = k; // at most one: validated
    }
  }
  if (found == p.n_expect || symbol < e[found].start_symbol || symbol >= (uint32_t)e[found].start_symbol + e[found].nof_symbols ||
      e[found].filter_index != 0) {
    return 17;
  }
  uint32_t port = 0;
  for (uint32_t k = 0; k != 4; ++k) {
    port = (k < p.n_ul_eaxc && p.ul_eaxc[k] == eaxc) ? k : port;
  }
  r.expect_index = found;
  r.grid_index   = e[found].grid_index;
  r.port         = (uint16_t)port;
  if (rb != 0) {
    return 18;
  }
  if (sym_inc != 0) {
    return 19;
  }
  if (start_prb < e[found].prb_start || start_prb + nof_prbs > (uint32_t)e[found].prb_start + e[found].nof_prb) {
    return 20;
  }
  // uplane_rx_symbol_data_flow_writer::write_to_resource_grid
  if (((e[found].context_symbols >> symbol) & 1u) == 0) {
    return 21;
  }
  const uint32_t du_nof_prbs = p.grid_nof_subc / 12u;
  r.nof_prbs_written         = (uint16_t)(start_prb >= du_nof_prbs ? 0u : min(nof_prbs, du_nof_prbs - start_prb));
  return 0;
}

struct OfhRxOwns {
  const uint32_t* own; // of the section's first PRB
  uint32_t        tag;
  __device__ __forceinline__ bool operator()(uint32_t prb) const { return own[prb] == tag; }
};

} // namespace

__global__ __launch_bounds__(256) void ofh_rx_parse_kernel(OfhRxLaunch p)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= p.n_frames) {
    return;
  }
  nrphy_ofh_rx_record_t r = {};
  r.status                = ofh_rx_parse(p, p.frames[i].offset, p.frames[i].length, r);
  p.records[i]            = r;
}

// sequence_id_checker_impl::update_and_compare_seq_id(eaxc, seq) on the lane's state word (bit 8: initialized, bits 0..7: the
// counter), applied only where `match`; returns the skipped count.  Without branches: the walk is one dependent chain per frame.
// The counter becomes seq for the first packet, for the expected one (a = 0) and for one from the future (a > 0), and stays for
// one from the past.
__device__ __forceinline__ int ofh_rx_check_seq_id(uint32_t& st, uint32_t seq, bool match)
{
  const bool initialized = (st & 0x100u) != 0;
  int        a           = (int)seq - (int)((st + 1u) & 0xFFu);
  a                      = a >= 128 ? a - 256 : (a < -128 ? a + 256 : a);
  a                      = initialized ? a : 0;
  st                     = (match && a >= 0) ? (0x100u | seq) : st;
  return a;
}

constexpr uint32_t OFH_RX_SEQ_TILE    = 4096; // frames whose words one pass holds in LDS
constexpr uint32_t OFH_RX_SEQ_THREADS = 1024;

__global__ __launch_bounds__(OFH_RX_SEQ_THREADS) void ofh_rx_sequence_kernel(OfhRxLaunch p)
{
  // Neither the walk, serial per eAxC, nor the claims may pay a trip to memory per frame, so both run from LDS, a tile of frames
  // at a time.  Walk: all threads fetch one word per frame (bit 31: the checker sees the frame; bits 8..10: its lane; bits 0..7:
  // the sequence identifier), lanes 0 .. n_eaxc - 1 of the first wave walk the words four at a time -- every lane reads the same
  // address, a broadcast -- and leave their answers in LDS, and all threads carry the answers back to the records.  Claims: thread
  // i fetches where frame i's PRBs are in the ownership table and how many it writes, then each wave takes every 16th frame and
  // issues its atomics, which nothing waits for.  Record i is read and written by thread i % 1024 alone.
  __shared__ __attribute__((aligned(16))) uint32_t s_word[OFH_RX_SEQ_TILE];
  __shared__ int                                   s_count[OFH_RX_SEQ_TILE];
  const uint32_t t = threadIdx.x, du_nof_prbs = p.grid_nof_subc / 12u;
  uint32_t       st = (p.seq_id_check && t < p.n_eaxc) ? p.state[t] : 0u;
  for (uint32_t base = 0; base < p.n_frames; base += OFH_RX_SEQ_TILE) {
    const uint32_t count = min(OFH_RX_SEQ_TILE, p.n_frames - base), padded = (count + 3u) & ~3u;
    if (p.seq_id_check) {
      for (uint32_t i = t; i < padded; i += OFH_RX_SEQ_THREADS) {
        uint32_t key = 0;
        if (i < count) {
          const nrphy_ofh_rx_record_t* r      = p.records + base + i;
          const uint32_t               status = r->status, eaxc = r->eaxc;
          uint32_t                     lane   = 0;
          for (uint32_t k = 0; k != OFH_RX_MAX_EAXC; ++k) {
            lane = (k < p.n_eaxc && p.eaxc[k] == eaxc) ? k : lane;
          }
          key = (status == 0 || status >= 8u) ? 0x80000000u | lane << 8 | (uint32_t)(r->seq_id >> 8) : 0u;
        }
        s_word[i] = key;
      }
      __syncthreads();
      if (t < p.n_eaxc) {
        for (uint32_t i = 0; i < padded; i += 4u) {
          const uint4    k4     = *reinterpret_cast<const uint4*>(s_word + i);
          const uint32_t key[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
          for (uint32_t j = 0; j != 4; ++j) {
            const bool match   = (key[j] >> 8) == (0x800000u | t);
            const int  skipped = ofh_rx_check_seq_id(st, key[j] & 0xFFu, match);
            if (match) {
              s_count[i + j] = skipped;
            }
          }
        }
      }
      __syncthreads();
      for (uint32_t i = t; i < count; i += OFH_RX_SEQ_THREADS) {
        if ((s_word[i] >> 31) == 0) {
          continue;
        }
        nrphy_ofh_rx_record_t* r       = p.records + base + i;
        const int              skipped = s_count[i];
        if (skipped < 0) { // from the past: nothing beyond the checker was reached
          nrphy_ofh_rx_record_t z = {};
          z.status                = 7;
          z.seq_skipped           = skipped;
          z.eaxc                  = r->eaxc;
          z.seq_id                = r->seq_id;
          *r                      = z;
        } else {
          r->seq_skipped = skipped;
        }
      }
      __syncthreads(); // the walk's words are spent
    }
    // the statuses are final
    for (uint32_t i = t; i < count; i += OFH_RX_SEQ_THREADS) {
      const nrphy_ofh_rx_record_t* r = p.records + base + i;
      const bool accepted            = r->status == 0;
      s_word[i]  = (uint32_t)((((size_t)r->grid_index * p.grid_nof_ports + r->port) * NRPHY_NSYMB + r->symbol) * du_nof_prbs + r->start_prb);
      s_count[i] = accepted ? (int)r->nof_prbs_written : 0;
    }
    __syncthreads();
    for (uint32_t i = t / WAVE; i < count; i += OFH_RX_SEQ_THREADS / WAVE) {
      const uint32_t written = (uint32_t)s_count[i];
      uint32_t*      own     = p.own + s_word[i];
      for (uint32_t prb = t % WAVE; prb < written; prb += WAVE) {
        atomicMax(own + prb, base + i + 1u);
      }
    }
    __syncthreads(); // before the next tile overwrites the words
  }
  if (p.seq_id_check && t < p.n_eaxc) {
    p.state[t] = st;
  }
}

__global__ __launch_bounds__(WAVE) void ofh_rx_write_kernel(OfhRxLaunch p)
{
  const uint32_t frame = blockIdx.x / p.chunks_per_frame, first = (blockIdx.x % p.chunks_per_frame) * OFH_UL_PRBS_PER_WG;
  const NRPHY_CONSTANT nrphy_ofh_rx_record_t* r = to_constant(p.records) + frame;
  const uint32_t written = r->nof_prbs_written;
  if (r->status != 0 || first >= written) {
    return;
  }
  const size_t row = ((size_t)r->grid_index * p.grid_nof_ports + r->port) * NRPHY_NSYMB + r->symbol;
  ofh_ul_chunk<false>(p.d_frames + r->payload_offset, first, min(OFH_UL_PRBS_PER_WG, written - first), 0u, 12u * written, r->data_width,
                      r->type, p.grid + row * p.grid_nof_subc + 12u * r->start_prb,
                      OfhRxOwns{p.own + row * (p.grid_nof_subc / 12u) + r->start_prb, frame + 1u});
}

hipError_t launch_ofh_rx(const OfhRxLaunch& p, hipStream_t stream)
{
  if (p.n_frames == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ofh_rx_parse_kernel, dim3((p.n_frames + 255u) / 256u), dim3(256), 0, stream, p);
  hipLaunchKernelGGL(ofh_rx_sequence_kernel, dim3(1), dim3(OFH_RX_SEQ_THREADS), 0, stream, p);
  if (p.chunks_per_frame != 0) {
    hipLaunchKernelGGL(ofh_rx_write_kernel, dim3(p.n_frames * p.chunks_per_frame), dim3(WAVE), 0, stream, p);
  }
  return hipGetLastError();
}

} // namespace nrphy
