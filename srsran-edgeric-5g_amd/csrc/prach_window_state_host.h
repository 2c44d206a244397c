// The device-free part of the PRACH window pipeline (prach_window_async.cpp): the order rules of a window -- which call is
// accepted when, and how many samples a run contributes -- whether a demodulator and a detector configuration describe the same
// PRACH, what a pool's limits admit, and the layout of a window's prach_buffer and of its result block, the same bytes on the
// device and in pinned memory.  Needs the public header alone (tests/prach_window_state_check.cpp compiles it by itself).  Not
// part of the ABI.
#pragma once

#include "mi355_nrphy.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

#pragma GCC visibility push(hidden)

// What a pool's configuration bounds, per window.
struct PrachWindowLimits {
  uint32_t max_window_samples = 0; // per port
  uint32_t max_ports = 0, max_td_occasions = 0, max_fd_occasions = 0;
};

// The dimensions of one open: what the two configurations and nrphy_prach_demod_sizes come to.
struct PrachWindowDims {
  uint32_t nof_ports = 0, nof_td = 0, nof_fd = 0, nof_symbols = 0, sequence_length = 0, window_samples = 0;
};

// The largest symbols x L_RA of an occasion: four symbols of 839 (formats 2 and 3); twelve of 139 (B4) are fewer.
constexpr size_t PRACH_WINDOW_MAX_OCCASION_ELEMS = 4 * 839;

inline size_t prach_window_align(size_t x, size_t a)
{
  return (x + a - 1) / a * a;
}

// The prach_buffer of a window is C-contiguous [port][td][fd][symbol][L_RA] complex f32 in the dimensions of its open: the
// element strides the two plans are made with, and what nrphy_prach_window_read_buffer copies out.
struct PrachWindowStrides {
  uint64_t port = 0, td = 0, fd = 0, symbol = 0, elems = 0;
};

inline PrachWindowStrides prach_window_strides(const PrachWindowDims& d)
{
  PrachWindowStrides s;
  s.symbol = d.sequence_length;
  s.fd     = s.symbol * d.nof_symbols;
  s.td     = s.fd * d.nof_fd;
  s.port   = s.td * d.nof_td;
  s.elems  = s.port * d.nof_ports;
  return s;
}

// Elements of the buffer a pool allocates per window: every open its limits admit fits.
inline size_t prach_window_buffer_elems(const PrachWindowLimits& lim)
{
  return (size_t)lim.max_ports * lim.max_td_occasions * lim.max_fd_occasions * PRACH_WINDOW_MAX_OCCASION_ELEMS;
}

// NRPHY_ERR_CAPACITY for an open beyond the pool's limits.
inline int prach_window_fits(const PrachWindowLimits& lim, const PrachWindowDims& d)
{
  if (d.window_samples > lim.max_window_samples || d.nof_ports > lim.max_ports || d.nof_td > lim.max_td_occasions ||
      d.nof_fd > lim.max_fd_occasions || prach_window_strides(d).elems > prach_window_buffer_elems(lim)) {
    return NRPHY_ERR_CAPACITY;
  }
  return NRPHY_OK;
}

// Byte offsets within a result block of n occasions, td outer: the result headers, then 64 preamble records per occasion on the
// next 64 bytes.  One copy of host_bytes brings both up.
struct PrachWindowLayout {
  size_t results = 0, preambles = 0, host_bytes = 0;
};

inline PrachWindowLayout prach_window_layout(uint32_t nof_occasions)
{
  PrachWindowLayout l;
  l.results    = 0;
  l.preambles  = prach_window_align((size_t)nof_occasions * sizeof(nrphy_prach_result_t), 64);
  l.host_bytes = l.preambles + (size_t)nof_occasions * NRPHY_PRACH_MAX_PREAMBLES * sizeof(nrphy_prach_preamble_t);
  return l;
}

// The block a pool allocates per window, on the device and pinned.
inline size_t prach_window_result_bytes(const PrachWindowLimits& lim)
{
  return prach_window_align(prach_window_layout(lim.max_td_occasions * lim.max_fd_occasions).host_bytes, 64);
}

// The RA spacing the demodulator derives from the format and the PUSCH numerology (get_prach_preamble_long_info / _short_info):
// 1.25 kHz for formats 0 to 2, 5 kHz for format 3, the PUSCH spacing for the short formats.
inline uint32_t prach_window_ra_scs(uint32_t format, uint32_t pusch_numerology)
{
  if (format <= NRPHY_PRACH_FORMAT_2) {
    return NRPHY_PRACH_SCS_1_25;
  }
  return format == NRPHY_PRACH_FORMAT_3 ? NRPHY_PRACH_SCS_5 : NRPHY_PRACH_SCS_15 + pusch_numerology;
}

// prach_processor_worker::handle_request hands ONE context to the demodulator and, through the buffer, to the detector.  Here the
// two halves arrive apart and must describe the same PRACH: format, RA spacing, receive ports, and the pool's sampling rate; and
// every PRACH port must map to a radio port the pool has.  Both configurations have passed their own validators.
inline int prach_window_pair_agrees(const nrphy_prach_demod_cfg_t& demod, const nrphy_prach_cfg_t& detect, const uint32_t* radio_port,
                                    uint32_t pool_srate_hz, uint32_t nof_radio_ports)
{
  if (demod.format != detect.format || detect.ra_scs != prach_window_ra_scs(demod.format, demod.pusch_numerology) ||
      demod.nof_rx_ports != detect.nof_rx_ports || demod.srate_hz != pool_srate_hz || radio_port == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t p = 0; p != demod.nof_rx_ports; ++p) {
    if (radio_port[p] >= nof_radio_ports) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  return NRPHY_OK;
}

// What a window's plans were made from: an open that brings the same bytes reuses them.
struct PrachWindowKey {
  nrphy_prach_demod_cfg_t demod;
  nrphy_prach_cfg_t       detect;
  uint32_t                radio_port[NRPHY_MAX_PORTS];
  bool                    valid = false;
};

inline void prach_window_key_set(PrachWindowKey& k, const nrphy_prach_demod_cfg_t& demod, const nrphy_prach_cfg_t& detect,
                                 const uint32_t* radio_port)
{
  std::memset(k.radio_port, 0, sizeof(k.radio_port));
  k.demod  = demod;
  k.detect = detect;
  std::memcpy(k.radio_port, radio_port, demod.nof_rx_ports * sizeof(uint32_t));
  k.valid = true;
}

inline bool prach_window_key_equal(const PrachWindowKey& k, const nrphy_prach_demod_cfg_t& demod, const nrphy_prach_cfg_t& detect,
                                   const uint32_t* radio_port)
{
  return k.valid && std::memcmp(&k.demod, &demod, sizeof(demod)) == 0 && std::memcmp(&k.detect, &detect, sizeof(detect)) == 0 &&
         std::memcmp(k.radio_port, radio_port, demod.nof_rx_ports * sizeof(uint32_t)) == 0;
}

// One open of a window.  A window is filled either by sample runs (prach_processor_worker::accumulate_samples) or by the caller
// on the device (split 7.2), never by both; the detector is enqueued once, by the run that completes the window or by
// nrphy_prach_window_buffer_written.
struct PrachWindowState {
  uint32_t window_length = 0; // samples per port: nrphy_prach_demod_sizes().window_samples
  uint32_t collected     = 0;
  bool     samples_seen  = false; // a sample run has been accepted (even one that took nothing)
  bool     written       = false; // nrphy_prach_window_buffer_written has been accepted
  bool     completed     = false; // the detector has been enqueued
};

inline void prach_window_state_open(PrachWindowState& s, uint32_t window_length)
{
  s               = PrachWindowState();
  s.window_length = window_length;
}

// A run of nof_samples per port: `taken` of them, from the front, belong to the window (0 and fewer than offered are no error).
inline int prach_window_accept_samples(const PrachWindowState& s, uint32_t nof_samples, uint32_t& taken)
{
  taken = 0;
  if (s.completed || s.written) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t left = s.window_length - s.collected;
  taken               = nof_samples < left ? nof_samples : left;
  return NRPHY_OK;
}

// After the run's copies have been enqueued; true when the window is complete and the caller enqueues the rest.
inline bool prach_window_commit_samples(PrachWindowState& s, uint32_t taken)
{
  s.samples_seen = true;
  s.collected += taken;
  if (s.collected == s.window_length) {
    s.completed = true;
  }
  return s.completed;
}

// Split 7.2: once per open, and not on a window that sample runs fill.
inline int prach_window_accept_buffer_written(const PrachWindowState& s)
{
  return s.completed || s.written || s.samples_seen ? NRPHY_ERR_ARGUMENT : NRPHY_OK;
}

inline void prach_window_commit_buffer_written(PrachWindowState& s)
{
  s.written   = true;
  s.completed = true;
}

#pragma GCC visibility pop
