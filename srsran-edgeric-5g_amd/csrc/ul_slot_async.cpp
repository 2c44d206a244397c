// The uplink slot pipeline (nrphy_ul_slots_* / nrphy_ul_slot_*): baseband samples to PUSCH, PUCCH and SRS results on one
// device-resident grid, the receive-side twin of dl_slot_async.cpp.
//
// The reference's lower PHY demodulates every port of one symbol into the slot's grid as soon as its samples are in
// (puxch_processor_impl::process_symbol, puxch_processor_impl.cpp:30-81) and notifies the upper PHY, which runs process_pusch,
// process_pucch and process_srs on that grid (uplink_processor_impl.cpp:86-170).  Here a run of symbols goes down in the radio's
// own sample format, nrphy_ofdm_demod_symbols writes its rows, and every receiver reads the grid where it is; the results of a
// slot collect in one device block whose layout ul_slot_state_host.h fixes, and one copy brings them up at finish.
//
// Rules as in dl_slot_async.cpp: a call enqueues copies and kernels on the slot's stream and returns; completion is a stream
// callback.  The receivers make their plans with the stand-alone *_plan_create (an allocation and a blocking upload each, under
// the context's host lock, as those calls are not written to run side by side on one context); the plans live until the slot is
// closed.
#include "nrphy_host_internal.h"
#include "slot_pool_host.h"
#include "ul_slot_state_host.h"

#include <cmath>
#include <new>

namespace {

// (the life cycle of slot_pool_host.h; the order of the calls on an open slot is ul_slot_state_host.h's)
struct UlSlot : SlotCore {
  nrphy_ul_slots* pool     = nullptr;
  hipStream_t     stream   = nullptr;
  uint32_t*       d_grid   = nullptr;
  uint8_t*        d_iq     = nullptr; // [port][slot_stride] samples
  uint8_t*        h_iq     = nullptr; // pinned twin
  uint8_t*        d_res    = nullptr; // the result block (UlSlotLayout)
  uint8_t*        h_res    = nullptr; // pinned: its first host_bytes
  void*           h_grid   = nullptr; // pinned: nrphy_ul_slot_load_grid / _read_grid
  bool            h_grid_busy = false; // a load of this open may still read h_grid
  uint32_t        slot_index  = 0;     // within the subframe
  UlSlotState     order;
  std::vector<nrphy_pusch_proc_plan_t*> pusch_plans; // of this open; destroyed at close
  std::vector<nrphy_pucch_plan_t*>      pucch_plans;
  std::vector<nrphy_pf2_plan_t*>        pf2_plans;
  std::vector<nrphy_srs_plan_t*>        srs_plans;
};

} // namespace

struct nrphy_ul_slots : SlotPool<UlSlot> {
  nrphy_ctx*              ctx = nullptr;
  nrphy_ul_slots_cfg_t    cfg;
  nrphy_ofdm_plan_t*      ofdm = nullptr;
  void*                   d_harq = nullptr;
  uint32_t                nof_subc = 0, slot_stride = 0, sample_bytes = 8, nsymb = 14;
  size_t                  grid_bytes = 0, iq_bytes = 0;
  UlSlotLayout            layout;
  std::vector<uint32_t>   sym_offset; // [slot of the subframe][nsymb + 1]: first sample of a symbol within its slot
  uint32_t*               d_slot_numbers = nullptr; // 0, 1, ... : the demodulator takes the slot index from device memory
};

namespace {

// Runs on a thread of the HIP runtime when the slot's results have reached the pinned block (or the stream has failed).
void on_slot_done(hipStream_t, hipError_t error, void* arg)
{
  UlSlot*         slot = static_cast<UlSlot*>(arg);
  nrphy_ul_slots* pool = slot->pool;
  // The UCI offsets of a result count from the PDU's own bits, as nrphy_pusch_proc_host gives them.
  auto* results = reinterpret_cast<nrphy_pusch_result_t*>(slot->h_res + pool->layout.pusch);
  for (uint32_t i = 0; i != slot->order.used.n_pusch; ++i) {
    const uint64_t at = slot->order.uci[i].at;
    results[i].harq_ack_offset -= results[i].nof_harq_ack != 0 ? at : 0;
    results[i].csi_part1_offset -= results[i].nof_csi_part1 != 0 ? at : 0;
  }
  slot_pool_complete(*pool, *slot, error == hipSuccess ? NRPHY_OK : NRPHY_ERR_DEVICE);
}

void destroy_plans(UlSlot& s)
{
  for (auto* p : s.pusch_plans) {
    nrphy_pusch_proc_plan_destroy(p);
  }
  for (auto* p : s.pucch_plans) {
    nrphy_pucch_plan_destroy(p);
  }
  for (auto* p : s.pf2_plans) {
    nrphy_pf2_plan_destroy(p);
  }
  for (auto* p : s.srs_plans) {
    nrphy_srs_plan_destroy(p);
  }
  s.pusch_plans.clear();
  s.pucch_plans.clear();
  s.pf2_plans.clear();
  s.srs_plans.clear();
}

// The gate of the four receiver calls: the slot of `slot_id`, locked, if it is open, not finished and the call brings items;
// otherwise no lock (NRPHY_ERR_ARGUMENT).
std::unique_lock<std::mutex> lock_for_receivers(nrphy_ul_slots* pool, uint32_t slot_id, uint32_t n, const void* items, UlSlot*& s)
{
  s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || n == 0 || items == nullptr) {
    return {};
  }
  std::unique_lock<std::mutex> lock(s->mutex);
  if (ul_slot_accept_open_call(s->order) != NRPHY_OK) {
    return {};
  }
  return lock;
}

// One item of a receiver call: its validator's status comes first, then whether its last symbol has been delivered.
int item_status(const UlSlot& s, int valid, uint32_t start_symbol, uint32_t nof_symbols)
{
  return valid != NRPHY_OK ? valid : ul_slot_accept_receiver(s.order, start_symbol, nof_symbols);
}

// What the tail of the four receiver calls starts with, once nothing of the call can be refused any more: the n items all read
// grid 0, the plan is made under the context's host lock, on the context's device (`device`: what hipSetDevice said).
struct PlanCall {
  const std::vector<uint32_t>           grid_of;
  std::lock_guard<std::recursive_mutex> host_lock;
  const hipError_t                      device;
  PlanCall(nrphy_ul_slots* pool, uint32_t n) : grid_of(n, 0), host_lock(pool->ctx->host_mutex), device(hipSetDevice(pool->ctx->device)) {}
};

} // namespace

extern "C" int nrphy_ul_slots_create(nrphy_ctx_t* ctx, const nrphy_ul_slots_cfg_t* cfg, void* d_harq, nrphy_ul_slots_t** out)
{
  if (ctx == nullptr || cfg == nullptr || out == nullptr || cfg->depth == 0 || cfg->depth > 64 || cfg->nof_ports == 0 ||
      cfg->nof_ports > NRPHY_MAX_PORTS || cfg->iq_format > NRPHY_IQ_CI16 || cfg->ofdm.bw_rb == 0 || cfg->ofdm.bw_rb > NRPHY_MAX_RB ||
      (cfg->iq_format == NRPHY_IQ_CI16 && !(cfg->iq_scale > 0.f && std::isfinite(cfg->iq_scale))) || ((uintptr_t)d_harq & 63U) != 0 ||
      cfg->max_pusch > 65535U || cfg->max_pucch > 65535U || cfg->max_pf2 > 65535U || cfg->max_srs > 65535U ||
      cfg->max_tb_bytes > (1U << 30) || cfg->max_uci_bits > (1U << 30)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  HIP_TRY(hipSetDevice(ctx->device));
  nrphy_ul_slots* pool = new (std::nothrow) nrphy_ul_slots;
  if (pool == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  pool->ctx    = ctx;
  pool->cfg    = *cfg;
  pool->d_harq = d_harq;
  int rc       = nrphy_ofdm_plan_create(ctx, &cfg->ofdm, cfg->nof_ports, &pool->ofdm);
  if (rc == NRPHY_OK && cfg->window_offset >= (144U * cfg->ofdm.dft_size) / 2048U) {
    rc = NRPHY_ERR_ARGUMENT; // as nrphy_ofdm_demod_run refuses it
  }
  if (rc != NRPHY_OK) {
    nrphy_ul_slots_destroy(pool);
    return rc;
  }
  pool->nsymb        = cfg->ofdm.cp ? 12 : 14;
  pool->nof_subc     = 12 * cfg->ofdm.bw_rb;
  pool->slot_stride  = nrphy_ofdm_plan_slot_stride(pool->ofdm);
  pool->sample_bytes = cfg->iq_format == NRPHY_IQ_CI16 ? 4 : 8;
  pool->grid_bytes   = (size_t)cfg->nof_ports * NRPHY_NSYMB * pool->nof_subc * 4;
  pool->iq_bytes     = (size_t)cfg->nof_ports * pool->slot_stride * pool->sample_bytes;
  UlSlotLimits lim;
  lim.nsymb        = pool->nsymb;
  lim.max_pusch    = cfg->max_pusch;
  lim.max_pucch    = cfg->max_pucch;
  lim.max_pf2      = cfg->max_pf2;
  lim.max_srs      = cfg->max_srs;
  lim.max_tb_bytes = cfg->max_tb_bytes;
  lim.max_uci_bits = cfg->max_uci_bits;
  pool->layout     = ul_slot_layout(lim);
  const uint32_t nof_slots = 1U << cfg->ofdm.numerology;
  pool->sym_offset.resize((size_t)nof_slots * (pool->nsymb + 1));
  std::vector<uint32_t> numbers(nof_slots);
  for (uint32_t slot = 0; slot != nof_slots; ++slot) {
    numbers[slot] = slot;
    uint32_t at   = 0;
    for (uint32_t l = 0; l <= pool->nsymb; ++l) {
      pool->sym_offset[(size_t)slot * (pool->nsymb + 1) + l] = at;
      at += nrphy_ofdm_symbol_size(&cfg->ofdm, slot * pool->nsymb + l);
    }
  }
  if (upload(&pool->d_slot_numbers, numbers.data(), numbers.size() * sizeof(uint32_t)) != hipSuccess) {
    nrphy_ul_slots_destroy(pool);
    return NRPHY_ERR_DEVICE;
  }
  pool->slots = std::vector<UlSlot>(cfg->depth);
  uint32_t id = 0;
  for (UlSlot& s : pool->slots) {
    s.pool = pool;
    s.id   = id++;
    ul_slot_state_init(s.order, lim);
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void**)&s.d_grid, pool->grid_bytes) != hipSuccess || hipMalloc((void**)&s.d_iq, pool->iq_bytes) != hipSuccess ||
        hipMalloc((void**)&s.d_res, pool->layout.total) != hipSuccess ||
        hipHostMalloc((void**)&s.h_iq, pool->iq_bytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&s.h_res, std::max<size_t>(pool->layout.host_bytes, 64), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&s.h_grid, pool->grid_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMemset(s.d_iq, 0, pool->iq_bytes) != hipSuccess) {
      nrphy_ul_slots_destroy(pool);
      return NRPHY_ERR_DEVICE;
    }
    s.pusch_plans.reserve(cfg->max_pusch);
    s.pucch_plans.reserve(cfg->max_pucch);
    s.pf2_plans.reserve(cfg->max_pf2);
    s.srs_plans.reserve(cfg->max_srs);
  }
  if (cfg->window_offset != 0) {
    // The demodulator builds the phase ramp of a window offset on first use (an allocation and a blocking upload): one launch
    // here, on samples that are all zero, keeps that off the sample path.
    UlSlot& s = pool->slots[0];
    rc        = nrphy_ofdm_demod_symbols(pool->ofdm, 1, s.d_iq, cfg->iq_format, cfg->iq_scale, pool->d_slot_numbers, 0, 1,
                                         cfg->window_offset, s.d_grid, s.stream);
    if (rc == NRPHY_OK && hipStreamSynchronize(s.stream) != hipSuccess) {
      rc = NRPHY_ERR_DEVICE;
    }
    if (rc != NRPHY_OK) {
      nrphy_ul_slots_destroy(pool);
      return rc;
    }
  }
  *out = pool;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slots_destroy(nrphy_ul_slots_t* pool)
{
  if (pool == nullptr) {
    return NRPHY_OK;
  }
  (void)hipSetDevice(pool->ctx->device);
  for (UlSlot& s : pool->slots) {
    if (s.stream) {
      (void)hipStreamSynchronize(s.stream); // callbacks included
    }
    destroy_plans(s);
    (void)hipFree(s.d_grid);
    (void)hipFree(s.d_iq);
    (void)hipFree(s.d_res);
    (void)hipHostFree(s.h_iq);
    (void)hipHostFree(s.h_res);
    (void)hipHostFree(s.h_grid);
    if (s.stream) {
      (void)hipStreamDestroy(s.stream);
    }
  }
  (void)hipFree(pool->d_slot_numbers);
  nrphy_ofdm_plan_destroy(pool->ofdm);
  delete pool;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slots_wait_free(nrphy_ul_slots_t* pool)
{
  return slot_pool_wait_free(pool);
}

extern "C" int nrphy_ul_slot_open(nrphy_ul_slots_t* pool, uint32_t subframe_slot_index, uint32_t* slot_id)
{
  if (pool == nullptr || slot_id == nullptr || subframe_slot_index >= (1U << pool->cfg.ofdm.numerology)) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlSlot* slot = slot_pool_claim(*pool);
  if (slot == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  std::lock_guard<std::mutex> lock(slot->mutex);
  ul_slot_state_open(slot->order);
  slot->slot_index  = subframe_slot_index;
  slot->h_grid_busy = false;
  // Symbols never delivered read as zero; a transport block whose CRC fails and the bytes a UCI decoder leaves alone likewise.
  if (hipSetDevice(pool->ctx->device) != hipSuccess || hipMemsetAsync(slot->d_grid, 0, pool->grid_bytes, slot->stream) != hipSuccess ||
      hipMemsetAsync(slot->d_res, 0, pool->layout.total, slot->stream) != hipSuccess) {
    slot_pool_release(*pool, *slot);
    return NRPHY_ERR_DEVICE;
  }
  *slot_id = slot->id;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_close(nrphy_ul_slots_t* pool, uint32_t slot_id)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  {
    std::lock_guard<std::mutex> lock(s->mutex);
    if (hipSetDevice(pool->ctx->device) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
      // (the slot is given back all the same: a failed stream fails the next use too, and says so)
    }
    // A completion callback of this slot may still be running on its runtime thread: wait for its state.
    slot_pool_await_callback(*pool, *s);
    destroy_plans(*s); // nothing of them is in flight any more
  }
  slot_pool_release(*pool, *s);
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_samples(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t first_symbol, uint32_t nof_symbols,
                                     const void* const* port_samples)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || port_samples == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(s->mutex);
  if (ul_slot_accept_samples(s->order, first_symbol, nof_symbols) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t port = 0; port != pool->cfg.nof_ports; ++port) {
    if (port_samples[port] == nullptr) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  // Everything that can refuse the run has been looked at (the format, the scale and the window offset when the pool was made,
  // the range just now): from here on only a device error ends the call early, and that fails the slot's stream with it.
  HIP_TRY(hipSetDevice(pool->ctx->device));
  const uint32_t* off   = &pool->sym_offset[(size_t)s->slot_index * (pool->nsymb + 1)];
  const size_t    at    = (size_t)off[first_symbol] * pool->sample_bytes;
  const size_t    bytes = (size_t)(off[first_symbol + nof_symbols] - off[first_symbol]) * pool->sample_bytes;
  for (uint32_t port = 0; port != pool->cfg.nof_ports; ++port) {
    const size_t here = (size_t)port * pool->slot_stride * pool->sample_bytes + at;
    std::memcpy(s->h_iq + here, port_samples[port], bytes);
  }
  for (uint32_t port = 0; port != pool->cfg.nof_ports; ++port) {
    const size_t here = (size_t)port * pool->slot_stride * pool->sample_bytes + at;
    HIP_TRY(hipMemcpyAsync(s->d_iq + here, s->h_iq + here, bytes, hipMemcpyHostToDevice, s->stream));
  }
  const int rc = nrphy_ofdm_demod_symbols(pool->ofdm, 1, s->d_iq, pool->cfg.iq_format, pool->cfg.iq_scale,
                                          pool->d_slot_numbers + s->slot_index, first_symbol, nof_symbols, pool->cfg.window_offset,
                                          s->d_grid, s->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->order.symbols = first_symbol + nof_symbols;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_load_grid(nrphy_ul_slots_t* pool, uint32_t slot_id, const void* grid)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || grid == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(s->mutex);
  if (ul_slot_accept_open_call(s->order) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(pool->ctx->device));
  // (h_grid may still feed an earlier load of this open: ordered behind it by waiting for the stream only then)
  if (s->h_grid_busy) {
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  std::memcpy(s->h_grid, grid, pool->grid_bytes);
  HIP_TRY(hipMemcpyAsync(s->d_grid, s->h_grid, pool->grid_bytes, hipMemcpyHostToDevice, s->stream));
  s->h_grid_busy   = true;
  s->order.symbols = s->order.lim.nsymb; // every symbol the slot has
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_symbols_written(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t upto)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(s->mutex);
  if (ul_slot_accept_symbols_written(s->order, upto) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  s->order.symbols = upto;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_pusch(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                   const nrphy_pusch_proc_options_t* options, const uint64_t* harq_soft_offset,
                                   const uint64_t* harq_state_offset)
{
  if (options == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_pusch_evm_options_t without_evm = {*options, 0, 0};
  return nrphy_pusch_evm_slot(pool, slot_id, n, pdus, &without_evm, harq_soft_offset, harq_state_offset);
}

extern "C" int nrphy_pusch_evm_slot(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                    const nrphy_pusch_evm_options_t* options, const uint64_t* harq_soft_offset,
                                    const uint64_t* harq_state_offset)
{
  return nrphy_pusch_tp_slot(pool, slot_id, n, pdus, nullptr, options, harq_soft_offset, harq_state_offset);
}

// The PUSCH operation of a slot; nrphy_pusch_evm_slot is this one without transform-precoding descriptors, nrphy_ul_slot_pusch
// that one with enable_evm = 0.
extern "C" int nrphy_pusch_tp_slot(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                   const nrphy_pusch_tp_desc_t* tps, const nrphy_pusch_evm_options_t* options,
                                   const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset)
{
  UlSlot*    s    = nullptr;
  const auto lock = lock_for_receivers(pool, slot_id, n, pdus, s);
  if (!lock || options == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlSlotUsed              used = s->order.used;
  std::vector<UlSlotSpan> tb(n), uci(n);
  std::vector<uint64_t>   tb_offset(n), uci_offset(n);
  for (uint32_t i = 0; i != n; ++i) {
    int rc = item_status(*s, nrphy_pusch_tp_validate(&pdus[i], tps != nullptr ? &tps[i] : nullptr, options, pool->cfg.nof_ports,
                                                     pool->nof_subc),
                         pdus[i].start_symbol_index, pdus[i].nof_symbols);
    if (rc != NRPHY_OK) {
      return rc;
    }
    if (pdus[i].has_codeword != 0 && (pool->d_harq == nullptr || harq_soft_offset == nullptr || harq_state_offset == nullptr)) {
      return NRPHY_ERR_ARGUMENT;
    }
    rc = ul_slot_take_pusch(s->order.lim, used, pdus[i].tb_size_bytes, pdus[i].nof_harq_ack + pdus[i].nof_csi_part1, tb[i], uci[i]);
    if (rc != NRPHY_OK) {
      return rc;
    }
    tb_offset[i]  = tb[i].at;
    uci_offset[i] = uci[i].at;
  }
  const PlanCall call(pool, n);
  HIP_TRY(call.device);
  nrphy_pusch_proc_plan_t* plan = nullptr;
  int rc = nrphy_pusch_tp_plan_create(pool->ctx, n, pdus, tps, options, call.grid_of.data(), 1, pool->cfg.nof_ports, pool->nof_subc,
                                      harq_soft_offset, harq_state_offset, tb_offset.data(), uci_offset.data(), &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->pusch_plans.push_back(plan);
  const uint32_t first = s->order.used.n_pusch;
  rc = nrphy_pusch_proc_run(plan, s->d_grid, pool->d_harq, s->d_res + pool->layout.tb, s->d_res + pool->layout.uci,
                            reinterpret_cast<nrphy_pusch_result_t*>(s->d_res + pool->layout.pusch) + first, s->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  for (uint32_t i = 0; i != n; ++i) {
    s->order.tb[first + i]  = tb[i];
    s->order.uci[first + i] = uci[i];
  }
  s->order.used = used;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_pf01(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pucch_cfg_t* cfgs)
{
  UlSlot*    s    = nullptr;
  const auto lock = lock_for_receivers(pool, slot_id, n, cfgs, s);
  if (!lock) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlSlotUsed used = s->order.used;
  for (uint32_t i = 0; i != n; ++i) {
    const int rc = item_status(*s, nrphy_pucch_validate(&cfgs[i], pool->cfg.nof_ports, pool->nof_subc), cfgs[i].start_symbol_index,
                               cfgs[i].nof_symbols);
    if (rc != NRPHY_OK) {
      return rc;
    }
  }
  int rc = ul_slot_take_count(s->order.lim.max_pucch, used.n_pucch, n);
  if (rc != NRPHY_OK) {
    return rc;
  }
  const PlanCall call(pool, n);
  HIP_TRY(call.device);
  nrphy_pucch_plan_t* plan = nullptr;
  rc = nrphy_pucch_plan_create(pool->ctx, n, cfgs, call.grid_of.data(), 1, pool->cfg.nof_ports, pool->nof_subc, nullptr, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->pucch_plans.push_back(plan);
  rc = nrphy_pucch_run(plan, s->d_grid, reinterpret_cast<nrphy_pucch_result_t*>(s->d_res + pool->layout.pucch) + s->order.used.n_pucch,
                       nullptr, nullptr, s->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->order.used = used;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_pf2(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_pf2_cfg_t* cfgs)
{
  UlSlot*    s    = nullptr;
  const auto lock = lock_for_receivers(pool, slot_id, n, cfgs, s);
  if (!lock) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlSlotUsed              used  = s->order.used;
  const uint32_t          first = used.n_pf2;
  std::vector<UlSlotSpan> msg(n);
  std::vector<uint64_t>   llr_offset(n), message_offset(n);
  for (uint32_t i = 0; i != n; ++i) {
    int rc = item_status(*s, nrphy_pf2_validate(&cfgs[i], pool->cfg.nof_ports, pool->nof_subc), cfgs[i].start_symbol_index,
                         cfgs[i].nof_symbols);
    if (rc != NRPHY_OK) {
      return rc;
    }
    uint32_t nof_llr = 0, nof_bits = 0;
    if (nrphy_pf2_sizes(&cfgs[i], &nof_llr, &nof_bits) != NRPHY_OK || nof_llr > UL_SLOT_PF2_LLR_BYTES) {
      return NRPHY_ERR_ARGUMENT;
    }
    rc = ul_slot_take_pf2(s->order.lim, used, nof_bits, msg[i]);
    if (rc != NRPHY_OK) {
      return rc;
    }
    llr_offset[i]     = (uint64_t)(first + i) * UL_SLOT_PF2_LLR_BYTES;
    message_offset[i] = msg[i].at;
  }
  const PlanCall call(pool, n);
  HIP_TRY(call.device);
  nrphy_pf2_plan_t* plan = nullptr;
  int rc = nrphy_pf2_plan_create(pool->ctx, n, cfgs, call.grid_of.data(), 1, pool->cfg.nof_ports, pool->nof_subc, llr_offset.data(),
                                 message_offset.data(), nullptr, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->pf2_plans.push_back(plan);
  rc = nrphy_pf2_run(plan, s->d_grid, reinterpret_cast<int8_t*>(s->d_res + pool->layout.pf2_llr), s->d_res + pool->layout.uci,
                     reinterpret_cast<uint32_t*>(s->d_res + pool->layout.pf2_status) + first,
                     reinterpret_cast<nrphy_pf2_csi_t*>(s->d_res + pool->layout.pf2_csi) + first, nullptr, nullptr, s->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  for (uint32_t i = 0; i != n; ++i) {
    s->order.pf2_msg[first + i] = msg[i];
  }
  s->order.used = used;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_srs(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t n, const nrphy_srs_cfg_t* cfgs)
{
  UlSlot*    s    = nullptr;
  const auto lock = lock_for_receivers(pool, slot_id, n, cfgs, s);
  if (!lock) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlSlotUsed used = s->order.used;
  for (uint32_t i = 0; i != n; ++i) {
    const int rc = item_status(*s, nrphy_srs_validate(&cfgs[i], pool->cfg.nof_ports, pool->nof_subc), cfgs[i].start_symbol,
                               cfgs[i].nof_symbols);
    if (rc != NRPHY_OK) {
      return rc;
    }
  }
  int rc = ul_slot_take_count(s->order.lim.max_srs, used.n_srs, n);
  if (rc != NRPHY_OK) {
    return rc;
  }
  const PlanCall call(pool, n);
  HIP_TRY(call.device);
  nrphy_srs_plan_t* plan = nullptr;
  rc = nrphy_srs_plan_create(pool->ctx, n, cfgs, call.grid_of.data(), 1, pool->cfg.nof_ports, pool->nof_subc, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->srs_plans.push_back(plan);
  rc = nrphy_srs_run(plan, s->d_grid, reinterpret_cast<nrphy_srs_result_t*>(s->d_res + pool->layout.srs) + s->order.used.n_srs, s->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  s->order.used = used;
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_finish(nrphy_ul_slots_t* pool, uint32_t slot_id, nrphy_ul_slot_done_fn done, void* user)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(s->mutex);
  if (ul_slot_accept_open_call(s->order) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT; // once per open
  }
  HIP_TRY(hipSetDevice(pool->ctx->device));
  s->order.finished = true;
  slot_arm(*s, done, user);
  if ((pool->layout.host_bytes != 0 &&
       hipMemcpyAsync(s->h_res, s->d_res, pool->layout.host_bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess) ||
      hipStreamAddCallback(s->stream, on_slot_done, s, 0) != hipSuccess) {
    (void)hipStreamSynchronize(s->stream);
    slot_fail_armed(*s);
    return NRPHY_ERR_DEVICE;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ul_slot_poll(nrphy_ul_slots_t* pool, uint32_t slot_id)
{
  return slot_pool_poll(pool, slot_id);
}

extern "C" int nrphy_ul_slot_wait(nrphy_ul_slots_t* pool, uint32_t slot_id)
{
  return slot_pool_wait(pool, slot_id);
}

extern "C" int nrphy_ul_slot_read_grid(nrphy_ul_slots_t* pool, uint32_t slot_id, void* grid)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || grid == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::lock_guard<std::mutex> lock(s->mutex);
  HIP_TRY(hipSetDevice(pool->ctx->device));
  HIP_TRY(hipMemcpyAsync(s->h_grid, s->d_grid, pool->grid_bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->h_grid_busy = false;
  std::memcpy(grid, s->h_grid, pool->grid_bytes);
  return NRPHY_OK;
}

extern "C" void* nrphy_ul_slot_device_grid(nrphy_ul_slots_t* pool, uint32_t slot_id)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  return s ? s->d_grid : nullptr;
}

extern "C" void* nrphy_ul_slot_stream(nrphy_ul_slots_t* pool, uint32_t slot_id)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  return s ? (void*)s->stream : nullptr;
}

// ---- accessors: pointer arithmetic into the pinned result block ------------------------------------------------------------
extern "C" const nrphy_pusch_result_t* nrphy_ul_slot_pusch_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || n == nullptr) {
    return nullptr;
  }
  *n = s->order.used.n_pusch;
  return reinterpret_cast<const nrphy_pusch_result_t*>(s->h_res + pool->layout.pusch);
}

extern "C" const uint8_t* nrphy_ul_slot_tb(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, uint32_t* nbytes)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || nbytes == nullptr || i >= s->order.used.n_pusch) {
    return nullptr;
  }
  *nbytes = s->order.tb[i].size;
  return s->h_res + pool->layout.tb + s->order.tb[i].at;
}

extern "C" const uint8_t* nrphy_ul_slot_pusch_uci(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, uint32_t* nbits)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || nbits == nullptr || i >= s->order.used.n_pusch) {
    return nullptr;
  }
  *nbits = s->order.uci[i].size;
  return s->h_res + pool->layout.uci + s->order.uci[i].at;
}

extern "C" const nrphy_pucch_result_t* nrphy_ul_slot_pf01_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || n == nullptr) {
    return nullptr;
  }
  *n = s->order.used.n_pucch;
  return reinterpret_cast<const nrphy_pucch_result_t*>(s->h_res + pool->layout.pucch);
}

extern "C" int nrphy_ul_slot_format2_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t i, const uint8_t** message, uint32_t* nbits,
                                         uint32_t* status, nrphy_pf2_csi_t* csi)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || i >= s->order.used.n_pf2) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (message != nullptr) {
    *message = s->h_res + pool->layout.uci + s->order.pf2_msg[i].at;
  }
  if (nbits != nullptr) {
    *nbits = s->order.pf2_msg[i].size;
  }
  if (status != nullptr) {
    *status = reinterpret_cast<const uint32_t*>(s->h_res + pool->layout.pf2_status)[i];
  }
  if (csi != nullptr) {
    *csi = reinterpret_cast<const nrphy_pf2_csi_t*>(s->h_res + pool->layout.pf2_csi)[i];
  }
  return NRPHY_OK;
}

extern "C" const nrphy_srs_result_t* nrphy_ul_slot_sounding_results(nrphy_ul_slots_t* pool, uint32_t slot_id, uint32_t* n)
{
  UlSlot* s = slot_pool_lookup(pool, slot_id);
  if (s == nullptr || n == nullptr) {
    return nullptr;
  }
  *n = s->order.used.n_srs;
  return reinterpret_cast<const nrphy_srs_result_t*>(s->h_res + pool->layout.srs);
}
