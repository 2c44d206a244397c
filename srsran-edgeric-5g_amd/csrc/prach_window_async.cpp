// The PRACH window pipeline (nrphy_prach_windows_* / nrphy_prach_window_*): baseband samples to detected preambles with the
// prach_buffer staying on the device, the sibling of ul_slot_async.cpp for the uplink channel whose window is not a slot.
//
// The reference's prach_processor_worker takes a PRACH context (handle_request), appends the samples of symbol after symbol to
// a window buffer until get_prach_window_duration of them are there (accumulate_samples), then hands the window to the
// demodulator and notifies the upper PHY, whose detector reads the prach_buffer (prach_processor_worker.cpp:31-162).  Here a run of
// samples goes down in the radio's own format as it arrives; the run that completes the window enqueues
// nrphy_prach_window_demod_run and nrphy_prach_run on the window's stream, and one copy brings the detections up.
//
// Rules as in ul_slot_async.cpp: a call enqueues copies and kernels on the window's stream and returns; completion is a stream
// callback.  The plans come from the stand-alone *_plan_create (an allocation and a blocking upload each, under the context's host
// lock); a window keeps them across opens while its configurations stay the same bytes, which for PRACH is the life of a cell.
#include "nrphy_host_internal.h"
#include "prach_window_state_host.h"
#include "slot_pool_host.h"

#include <atomic>
#include <cmath>
#include <new>

namespace {

// (the life cycle of slot_pool_host.h; the order of the calls on an open window is prach_window_state_host.h's)
struct PrachWindow : SlotCore {
  nrphy_prach_windows*       pool   = nullptr;
  hipStream_t                stream = nullptr;
  uint8_t*                   d_iq   = nullptr; // [PRACH port][max_window_samples] samples
  uint8_t*                   h_iq   = nullptr; // pinned twin
  float2*                    d_buf  = nullptr; // the prach_buffer (PrachWindowStrides)
  uint8_t*                   d_res  = nullptr; // the result block (PrachWindowLayout)
  uint8_t*                   h_res  = nullptr; // pinned twin
  nrphy_prach_demod_plan_t*  demod  = nullptr; // of the last open that made plans
  nrphy_prach_plan_t*        detect = nullptr;
  PrachWindowKey             key;
  PrachWindowDims            dims;
  PrachWindowState           order;
  nrphy_prach_window_done_fn open_done = nullptr; // handed to slot_arm when the detector is enqueued
  void*                      open_user = nullptr;
};

} // namespace

struct nrphy_prach_windows : SlotPool<PrachWindow> {
  nrphy_ctx*                ctx = nullptr;
  nrphy_prach_windows_cfg_t cfg;
  PrachWindowLimits         lim;
  uint32_t                  sample_bytes = 8;
  size_t                    iq_bytes = 0, buf_bytes = 0, res_bytes = 0;
  std::atomic<uint64_t>     plans_made{0};
};

namespace {

// Runs on a thread of the HIP runtime when the window's results have reached the pinned block (or the stream has failed).
void on_window_done(hipStream_t, hipError_t error, void* arg)
{
  PrachWindow* w = static_cast<PrachWindow*>(arg);
  slot_pool_complete(*w->pool, *w, error == hipSuccess ? NRPHY_OK : NRPHY_ERR_DEVICE);
}

void destroy_plans(PrachWindow& w)
{
  nrphy_prach_demod_plan_destroy(w.demod);
  nrphy_prach_plan_destroy(w.detect);
  w.demod     = nullptr;
  w.detect    = nullptr;
  w.key.valid = false;
}

// A device error in a call that has begun to enqueue: the window ends here.  Nothing more is accepted, what is on the stream is
// waited for, and the window is DONE with NRPHY_ERR_DEVICE for poll and wait; no handler runs (slot_fail_armed).  The caller
// holds the window's mutex.
int fail_window(PrachWindow& w, int rc)
{
  w.order.completed = true;
  (void)hipStreamSynchronize(w.stream);
  if (slot_is_open(w)) {
    slot_arm(w, nullptr, nullptr);
  }
  slot_fail_armed(w);
  return rc;
}

// The tail of a window, after its buffer is (or will be, in stream order) full: the detector over every occasion, one copy of
// the result block, the callback.  The caller holds the window's mutex and has committed the order state.
int enqueue_detection(nrphy_prach_windows* pool, PrachWindow& w)
{
  const PrachWindowLayout l = prach_window_layout(w.dims.nof_td * w.dims.nof_fd);
  slot_arm(w, w.open_done, w.open_user);
  const int rc = nrphy_prach_run(w.detect, w.d_buf, reinterpret_cast<nrphy_prach_result_t*>(w.d_res + l.results),
                                 reinterpret_cast<nrphy_prach_preamble_t*>(w.d_res + l.preambles), nullptr, w.stream);
  if (rc != NRPHY_OK || hipMemcpyAsync(w.h_res, w.d_res, l.host_bytes, hipMemcpyDeviceToHost, w.stream) != hipSuccess ||
      hipStreamAddCallback(w.stream, on_window_done, &w, 0) != hipSuccess) {
    return fail_window(w, rc != NRPHY_OK ? rc : NRPHY_ERR_DEVICE);
  }
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_prach_windows_create(nrphy_ctx_t* ctx, const nrphy_prach_windows_cfg_t* cfg, nrphy_prach_windows_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || cfg == nullptr || cfg->srate_hz == 0 || cfg->nof_radio_ports == 0 || cfg->nof_radio_ports > 64 ||
      cfg->depth == 0 || cfg->depth > 16 || cfg->iq_format > NRPHY_IQ_CI16 || cfg->max_window_samples == 0 ||
      cfg->max_window_samples > (1U << 26) || (cfg->iq_format == NRPHY_IQ_CI16 && !(cfg->iq_scale > 0.f && std::isfinite(cfg->iq_scale))) ||
      cfg->max_ports == 0 || cfg->max_ports > NRPHY_MAX_PORTS || cfg->max_td_occasions == 0 || cfg->max_td_occasions > 7 ||
      cfg->max_fd_occasions == 0 || cfg->max_fd_occasions > 8) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  nrphy_prach_windows* pool = new (std::nothrow) nrphy_prach_windows;
  if (pool == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  pool->ctx                    = ctx;
  pool->cfg                    = *cfg;
  pool->lim.max_window_samples = cfg->max_window_samples;
  pool->lim.max_ports          = cfg->max_ports;
  pool->lim.max_td_occasions   = cfg->max_td_occasions;
  pool->lim.max_fd_occasions   = cfg->max_fd_occasions;
  pool->sample_bytes           = cfg->iq_format == NRPHY_IQ_CI16 ? 4 : 8;
  pool->iq_bytes               = (size_t)cfg->max_ports * cfg->max_window_samples * pool->sample_bytes;
  pool->buf_bytes              = prach_window_buffer_elems(pool->lim) * sizeof(float2);
  pool->res_bytes              = prach_window_result_bytes(pool->lim);
  pool->slots                  = std::vector<PrachWindow>(cfg->depth);
  uint32_t id                  = 0;
  for (PrachWindow& w : pool->slots) {
    w.pool = pool;
    w.id   = id++;
    if (hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&w.d_iq, pool->iq_bytes) != hipSuccess || hipMalloc((void**)&w.d_buf, pool->buf_bytes) != hipSuccess ||
        hipMalloc((void**)&w.d_res, pool->res_bytes) != hipSuccess ||
        hipHostMalloc((void**)&w.h_iq, pool->iq_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&w.h_res, pool->res_bytes, hipHostMallocDefault) != hipSuccess) {
      nrphy_prach_windows_destroy(pool);
      return NRPHY_ERR_DEVICE;
    }
  }
  *out = pool;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_windows_destroy(nrphy_prach_windows_t* pool)
{
  if (pool == nullptr) {
    return NRPHY_OK;
  }
  (void)hipSetDevice(pool->ctx->device);
  for (PrachWindow& w : pool->slots) {
    if (w.stream) {
      (void)hipStreamSynchronize(w.stream); // callbacks included
    }
    destroy_plans(w);
    (void)hipFree(w.d_iq);
    (void)hipFree(w.d_buf);
    (void)hipFree(w.d_res);
    (void)hipHostFree(w.h_iq);
    (void)hipHostFree(w.h_res);
    if (w.stream) {
      (void)hipStreamDestroy(w.stream);
    }
  }
  delete pool;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_windows_wait_free(nrphy_prach_windows_t* pool)
{
  return slot_pool_wait_free(pool);
}

extern "C" uint64_t nrphy_prach_windows_plans_made(nrphy_prach_windows_t* pool)
{
  return pool != nullptr ? pool->plans_made.load(std::memory_order_relaxed) : 0;
}

extern "C" int nrphy_prach_window_open(nrphy_prach_windows_t* pool, const nrphy_prach_demod_cfg_t* demod, const uint32_t* radio_port,
                                       const nrphy_prach_cfg_t* detect, nrphy_prach_window_done_fn done, void* user, uint32_t* window_id)
{
  nrphy_prach_demod_sizes_t sizes;
  if (pool == nullptr || window_id == nullptr || nrphy_prach_demod_sizes(demod, &sizes) != NRPHY_OK ||
      nrphy_prach_validate(detect) != NRPHY_OK ||
      prach_window_pair_agrees(*demod, *detect, radio_port, pool->cfg.srate_hz, pool->cfg.nof_radio_ports) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  PrachWindowDims dims;
  dims.nof_ports       = demod->nof_rx_ports;
  dims.nof_td          = demod->nof_td_occasions;
  dims.nof_fd          = demod->nof_fd_occasions;
  dims.nof_symbols     = sizes.nof_symbols;
  dims.sequence_length = sizes.sequence_length;
  dims.window_samples  = sizes.window_samples;
  if (prach_window_fits(pool->lim, dims) != NRPHY_OK) {
    return NRPHY_ERR_CAPACITY;
  }
  PrachWindow* w = slot_pool_claim(*pool);
  if (w == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  std::lock_guard<std::mutex> lock(w->mutex);
  const PrachWindowStrides    st = prach_window_strides(dims);
  int                         rc = hipSetDevice(pool->ctx->device) == hipSuccess ? NRPHY_OK : NRPHY_ERR_DEVICE;
  if (rc == NRPHY_OK && !prach_window_key_equal(w->key, *demod, *detect, radio_port)) {
    // Nothing of this window is in flight (close has waited), so its old plans can go.
    std::lock_guard<std::recursive_mutex> host_lock(pool->ctx->host_mutex);
    destroy_plans(*w);
    const uint64_t                 zero = 0;
    const uint32_t                 nof_occasions = dims.nof_td * dims.nof_fd;
    std::vector<nrphy_prach_cfg_t> cfgs(nof_occasions, *detect);
    std::vector<uint64_t>          sym_offset(nof_occasions);
    for (uint32_t td = 0; td != dims.nof_td; ++td) {
      for (uint32_t fd = 0; fd != dims.nof_fd; ++fd) {
        sym_offset[td * dims.nof_fd + fd] = td * st.td + fd * st.fd;
      }
    }
    rc = nrphy_prach_demod_plan_create(pool->ctx, 1, demod, &zero, pool->cfg.max_window_samples, &zero, st.port, st.fd, st.td, st.symbol,
                                       &w->demod);
    if (rc == NRPHY_OK) {
      rc = nrphy_prach_plan_create(pool->ctx, nof_occasions, cfgs.data(), sym_offset.data(), st.port, st.symbol, &w->detect);
    }
    if (rc == NRPHY_OK) {
      prach_window_key_set(w->key, *demod, *detect, radio_port);
      pool->plans_made.fetch_add(1, std::memory_order_relaxed);
    } else {
      destroy_plans(*w);
    }
  }
  // Elements the split-7.2 writer never reaches read as zero, not as the window before.
  if (rc == NRPHY_OK && hipMemsetAsync(w->d_buf, 0, st.elems * sizeof(float2), w->stream) != hipSuccess) {
    rc = NRPHY_ERR_DEVICE;
  }
  if (rc != NRPHY_OK) {
    slot_pool_release(*pool, *w);
    return rc;
  }
  w->dims      = dims;
  w->open_done = done;
  w->open_user = user;
  prach_window_state_open(w->order, dims.window_samples);
  *window_id = w->id;
  return NRPHY_OK;
}

extern "C" int nrphy_prach_window_close(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  if (w == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  {
    std::lock_guard<std::mutex> lock(w->mutex);
    if (hipSetDevice(pool->ctx->device) != hipSuccess || hipStreamSynchronize(w->stream) != hipSuccess) {
      // (the window is given back all the same: a failed stream fails the next use too, and says so)
    }
    // A completion callback of this window may still be running on its runtime thread: wait for its state.
    slot_pool_await_callback(*pool, *w);
  }
  slot_pool_release(*pool, *w);
  return NRPHY_OK;
}

extern "C" int nrphy_prach_window_samples(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t nof_samples,
                                          const void* const* radio_port_samples, uint32_t* taken)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  if (w == nullptr || radio_port_samples == nullptr || taken == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *taken = 0;
  std::lock_guard<std::mutex> lock(w->mutex);
  uint32_t                    n = 0;
  if (prach_window_accept_samples(w->order, nof_samples, n) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t p = 0; p != w->dims.nof_ports; ++p) {
    if (radio_port_samples[w->key.radio_port[p]] == nullptr) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  // Everything that can refuse the run has been looked at: from here on only a device error ends the call early, and that ends
  // the window with it (fail_window).
  HIP_TRY(hipSetDevice(pool->ctx->device));
  const size_t at = (size_t)w->order.collected * pool->sample_bytes, bytes = (size_t)n * pool->sample_bytes;
  if (n != 0) {
    for (uint32_t p = 0; p != w->dims.nof_ports; ++p) {
      const size_t here = (size_t)p * pool->cfg.max_window_samples * pool->sample_bytes + at;
      std::memcpy(w->h_iq + here, radio_port_samples[w->key.radio_port[p]], bytes);
    }
    for (uint32_t p = 0; p != w->dims.nof_ports; ++p) {
      const size_t here = (size_t)p * pool->cfg.max_window_samples * pool->sample_bytes + at;
      if (hipMemcpyAsync(w->d_iq + here, w->h_iq + here, bytes, hipMemcpyHostToDevice, w->stream) != hipSuccess) {
        return fail_window(*w, NRPHY_ERR_DEVICE);
      }
    }
  }
  *taken = n;
  if (!prach_window_commit_samples(w->order, n)) {
    return NRPHY_OK;
  }
  const int rc = nrphy_prach_window_demod_run(w->demod, w->d_iq, pool->cfg.iq_format, pool->cfg.iq_scale, w->d_buf, w->stream);
  if (rc != NRPHY_OK) {
    return fail_window(*w, rc);
  }
  return enqueue_detection(pool, *w);
}

extern "C" void* nrphy_prach_window_device_buffer(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  return w ? (void*)w->d_buf : nullptr;
}

extern "C" void* nrphy_prach_window_stream(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  return w ? (void*)w->stream : nullptr;
}

extern "C" int nrphy_prach_window_buffer_written(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  if (w == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(w->mutex);
  if (prach_window_accept_buffer_written(w->order) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(pool->ctx->device));
  prach_window_commit_buffer_written(w->order);
  return enqueue_detection(pool, *w);
}

extern "C" int nrphy_prach_window_poll(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  return slot_pool_poll(pool, window_id);
}

extern "C" int nrphy_prach_window_wait(nrphy_prach_windows_t* pool, uint32_t window_id)
{
  return slot_pool_wait(pool, window_id);
}

extern "C" int nrphy_prach_window_read_buffer(nrphy_prach_windows_t* pool, uint32_t window_id, void* symbols)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  if (w == nullptr || symbols == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(w->mutex);
  HIP_TRY(hipSetDevice(pool->ctx->device));
  HIP_TRY(hipStreamSynchronize(w->stream));
  HIP_TRY(hipMemcpy(symbols, w->d_buf, prach_window_strides(w->dims).elems * sizeof(float2), hipMemcpyDeviceToHost));
  return NRPHY_OK;
}

// ---- accessors: pointer arithmetic into the pinned result block ------------------------------------------------------------
extern "C" const nrphy_prach_result_t* nrphy_prach_window_results(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t* n)
{
  PrachWindow* w = slot_pool_lookup(pool, window_id);
  if (w == nullptr || n == nullptr || slot_pool_poll(pool, window_id) != NRPHY_OK) { // valid from completion
    return nullptr;
  }
  *n = w->dims.nof_td * w->dims.nof_fd;
  return reinterpret_cast<const nrphy_prach_result_t*>(w->h_res + prach_window_layout(*n).results);
}

extern "C" const nrphy_prach_preamble_t* nrphy_prach_window_preambles(nrphy_prach_windows_t* pool, uint32_t window_id, uint32_t occasion)
{
  PrachWindow*   w = slot_pool_lookup(pool, window_id);
  const uint32_t n = w != nullptr && slot_pool_poll(pool, window_id) == NRPHY_OK ? w->dims.nof_td * w->dims.nof_fd : 0;
  if (occasion >= n) {
    return nullptr;
  }
  return reinterpret_cast<const nrphy_prach_preamble_t*>(w->h_res + prach_window_layout(n).preambles) + (size_t)occasion * NRPHY_PRACH_MAX_PREAMBLES;
}
