// The device-free part of the uplink slot pipeline (ul_slot_async.cpp): the order rules of a slot -- which call is accepted
// when -- and the layout of a slot's result block, the same bytes on the device and in pinned memory.  Needs the public header
// alone (tests/ul_slot_state_check.cpp compiles it by itself).  Not part of the ABI.
#pragma once

#include "mi355_nrphy.h"

#include <cstddef>
#include <cstdint>
#include <vector>

#pragma GCC visibility push(hidden)

// What a pool's configuration bounds, per slot.
struct UlSlotLimits {
  uint32_t nsymb        = 14; // symbols per slot: 12 with extended cyclic prefix
  uint32_t max_pusch    = 0, max_pucch = 0, max_pf2 = 0, max_srs = 0;
  uint32_t max_tb_bytes = 0, max_uci_bits = 0;
};

// A format 2 PUCCH has at most 16 PRB x 2 symbols x 8 data RE x 2 bits: the soft bits of PUCCH i are at llr + i * this.
constexpr size_t UL_SLOT_PF2_LLR_BYTES = 16 * 2 * 8 * 2;

// Byte offsets of the sections of a result block.  Every section starts on 64 bytes (the result structures need 8).  What the
// host reads lies in front, [0, host_bytes): one copy brings it up; the soft bits of format 2 stay on the device behind it.
struct UlSlotLayout {
  size_t pusch = 0, pucch = 0, pf2_status = 0, pf2_csi = 0, srs = 0, tb = 0, uci = 0, host_bytes = 0, pf2_llr = 0, total = 0;
};

inline size_t ul_slot_align(size_t x, size_t a)
{
  return (x + a - 1) / a * a;
}

// Transport block i starts on a 4-byte boundary, so the blocks of max_pusch PDUs take up to 3 bytes each beyond max_tb_bytes.
inline size_t ul_slot_tb_region_bytes(const UlSlotLimits& lim)
{
  return ul_slot_align(lim.max_tb_bytes, 4) + (size_t)4 * lim.max_pusch;
}

inline UlSlotLayout ul_slot_layout(const UlSlotLimits& lim)
{
  UlSlotLayout l;
  size_t       at = 0;
  auto         take = [&at](size_t bytes) {
    const size_t here = at;
    at                = ul_slot_align(at + bytes, 64);
    return here;
  };
  l.pusch      = take((size_t)lim.max_pusch * sizeof(nrphy_pusch_result_t));
  l.pucch      = take((size_t)lim.max_pucch * sizeof(nrphy_pucch_result_t));
  l.pf2_status = take((size_t)lim.max_pf2 * sizeof(uint32_t));
  l.pf2_csi    = take((size_t)lim.max_pf2 * sizeof(nrphy_pf2_csi_t));
  l.srs        = take((size_t)lim.max_srs * sizeof(nrphy_srs_result_t));
  l.tb         = take(ul_slot_tb_region_bytes(lim));
  l.uci        = take(lim.max_uci_bits);
  l.host_bytes = at;
  l.pf2_llr    = take((size_t)lim.max_pf2 * UL_SLOT_PF2_LLR_BYTES);
  l.total      = at > 64 ? at : 64;
  return l;
}

// A span of the transport-block or the UCI region.
struct UlSlotSpan {
  uint32_t at = 0, size = 0;
};

// One open of a slot: what has been delivered and what the receiver calls so far have taken.  A call is checked with the
// functions below on a COPY of `used`; the caller commits the copy once everything of the call has been enqueued, so a refused
// call leaves no trace.
struct UlSlotUsed {
  uint32_t n_pusch = 0, n_pucch = 0, n_pf2 = 0, n_srs = 0;
  uint32_t tb_bytes = 0; // transport-block bytes taken (what max_tb_bytes bounds)
  uint32_t tb_at    = 0; // where the next block starts: a multiple of 4
  uint32_t uci_at   = 0; // UCI bits taken, one byte each: PUSCH payloads and format 2 messages share the region
};
struct UlSlotState {
  UlSlotLimits            lim;
  uint32_t                symbols  = 0;     // symbols [0, symbols) are in the grid
  bool                    finished = false; // nrphy_ul_slot_finish has been accepted
  UlSlotUsed              used;
  std::vector<UlSlotSpan> tb, uci, pf2_msg; // per PUSCH PDU, per PUSCH PDU, per format 2 PUCCH (sized once, at creation)
};

inline void ul_slot_state_init(UlSlotState& s, const UlSlotLimits& lim)
{
  s.lim = lim;
  s.tb.assign(lim.max_pusch, UlSlotSpan());
  s.uci.assign(lim.max_pusch, UlSlotSpan());
  s.pf2_msg.assign(lim.max_pf2, UlSlotSpan());
  s.symbols  = 0;
  s.finished = false;
  s.used     = UlSlotUsed();
}

// nrphy_ul_slot_open: nothing delivered, nothing taken.
inline void ul_slot_state_open(UlSlotState& s)
{
  s.symbols  = 0;
  s.finished = false;
  s.used     = UlSlotUsed();
}

// A run of sample symbols: contiguous, in order, starting at 0, inside the slot.
inline int ul_slot_accept_samples(const UlSlotState& s, uint32_t first_symbol, uint32_t nof_symbols)
{
  if (s.finished || nof_symbols == 0 || first_symbol != s.symbols || first_symbol >= s.lim.nsymb ||
      nof_symbols > s.lim.nsymb - first_symbol) {
    return NRPHY_ERR_ARGUMENT;
  }
  return NRPHY_OK;
}

// nrphy_ul_slot_symbols_written: the count only grows and stays inside the symbols a slot has (12 with extended cyclic prefix),
// so that `symbols` never exceeds lim.nsymb whichever way the grid is filled.
inline int ul_slot_accept_symbols_written(const UlSlotState& s, uint32_t upto)
{
  return s.finished || upto < s.symbols || upto > s.lim.nsymb ? NRPHY_ERR_ARGUMENT : NRPHY_OK;
}

// A grid writer other than the demodulator (load_grid), and finish itself.
inline int ul_slot_accept_open_call(const UlSlotState& s)
{
  return s.finished ? NRPHY_ERR_ARGUMENT : NRPHY_OK;
}

// A receiver whose allocation is symbols [start, start + nof): its last symbol must have been delivered.
inline int ul_slot_accept_receiver(const UlSlotState& s, uint32_t start_symbol, uint32_t nof_symbols)
{
  if (s.finished || nof_symbols == 0 || (uint64_t)start_symbol + nof_symbols > s.symbols) {
    return NRPHY_ERR_ARGUMENT;
  }
  return NRPHY_OK;
}

// One PUSCH PDU with a transport block of tb_bytes (0: none) and uci_bits payload bits.
inline int ul_slot_take_pusch(const UlSlotLimits& lim, UlSlotUsed& u, uint32_t tb_bytes, uint32_t uci_bits, UlSlotSpan& tb, UlSlotSpan& uci)
{
  if (u.n_pusch >= lim.max_pusch || tb_bytes > lim.max_tb_bytes - u.tb_bytes || uci_bits > lim.max_uci_bits - u.uci_at) {
    return NRPHY_ERR_CAPACITY;
  }
  tb.at    = u.tb_at;
  tb.size  = tb_bytes;
  uci.at   = u.uci_at;
  uci.size = uci_bits;
  ++u.n_pusch;
  u.tb_bytes += tb_bytes;
  u.tb_at = (uint32_t)ul_slot_align((size_t)u.tb_at + tb_bytes, 4);
  u.uci_at += uci_bits;
  return NRPHY_OK;
}

// One format 2 PUCCH with a message of msg_bits.
inline int ul_slot_take_pf2(const UlSlotLimits& lim, UlSlotUsed& u, uint32_t msg_bits, UlSlotSpan& msg)
{
  if (u.n_pf2 >= lim.max_pf2 || msg_bits > lim.max_uci_bits - u.uci_at) {
    return NRPHY_ERR_CAPACITY;
  }
  msg.at   = u.uci_at;
  msg.size = msg_bits;
  ++u.n_pf2;
  u.uci_at += msg_bits;
  return NRPHY_OK;
}

// n results of fixed size: format 0 / 1 PUCCHs and SRS.
inline int ul_slot_take_count(uint32_t max, uint32_t& used, uint32_t n)
{
  if (n > max - used) {
    return NRPHY_ERR_CAPACITY;
  }
  used += n;
  return NRPHY_OK;
}

#pragma GCC visibility pop
