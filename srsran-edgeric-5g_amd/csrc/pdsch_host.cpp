// The device side of the PDSCH plan behind the C ABI of include/mi355_nrphy.h: where the tables that pdsch_plan_build.cpp
// builds live (an allocation of the plan's own, or memory the caller placed), the plan's streams and events, the launches of
// a run, its timing, and the host-span forms.  No compute happens here and there is no CPU fallback.
#include "pdsch_plan.h"
#include "nrphy_trace.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

namespace {

// The one owner of a plan from its creation on, a half-built one included: nrphy_pdsch_plan_destroy is safe on a plan without
// device memory, streams or events.
struct PlanDestroy {
  void operator()(nrphy_pdsch_plan* plan) const { (void)nrphy_pdsch_plan_destroy(plan); }
};
using PlanHandle = std::unique_ptr<nrphy_pdsch_plan, PlanDestroy>;

// Side streams the codeblock launches of the plan take under `dispatch` (Tunables::cb_dispatch): one per non-empty bucket
// beyond the first where the launcher takes one launch per bucket (launch_codeblocks), none where it takes the mixed kernel.
uint32_t side_streams_wanted(const nrphy_pdsch_plan* plan, int dispatch)
{
  PdschLaunch p;
  p.n_work             = plan->n_work;
  uint32_t nof_buckets = 0;
  if (!codeblocks_take_bucket_launches(p, plan->bucket_begin, dispatch, &nof_buckets) || nof_buckets < 2) {
    return 0;
  }
  return std::min<uint32_t>(nof_buckets - 1, nrphy_pdsch_plan::MAX_AUX);
}

// The plan's side streams and fork / join events for bucket launches that run side by side (nrphy_pdsch_run).
bool plan_side_streams(nrphy_pdsch_plan* plan, uint32_t want)
{
  while (plan->n_aux < want) {
    const uint32_t k = plan->n_aux;
    if (plan->fork_event == nullptr && hipEventCreateWithFlags(&plan->fork_event, hipEventDisableTiming) != hipSuccess) {
      return false;
    }
    if (hipStreamCreateWithFlags(&plan->aux_stream[k], hipStreamNonBlocking) != hipSuccess) {
      return false;
    }
    if (hipEventCreateWithFlags(&plan->join_event[k], hipEventDisableTiming) != hipSuccess) {
      (void)hipStreamDestroy(plan->aux_stream[k]);
      return false;
    }
    ++plan->n_aux;
  }
  return true;
}

// A plan from the builder, with a home for its tables: device memory of the plan's own, filled by one blocking copy, or
// (place != nullptr) memory the caller owns, with no HIP call at all.
int plan_create(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint64_t* tb_offset,
                const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                const EncodeOnly* enc, nrphy_pdsch_plan_t** out, PlanPlacement* place = nullptr)
{
  if (ctx == nullptr || out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  PlanHandle plan(new (std::nothrow) nrphy_pdsch_plan);
  if (plan == nullptr) {
    return NRPHY_ERR_CAPACITY;
  }
  plan->ctx            = ctx;
  plan->arena_external = place != nullptr; // (from the start: destroying a placed plan, a refused one too, makes no HIP call)
  PlanTables t;
  const int  status = pdsch_plan_build(ctx->graphs.data(), ctx->tune, n_pdu, pdus, tb_offset, grid_index, nof_grids, grid_nof_ports,
                                       grid_nof_subc, enc, place ? place->cache : nullptr,
                                       place ? place->scratch_capacity_words : 0, *plan, t);
  if (status != NRPHY_OK) {
    return status;
  }
  DeviceArena arena;
  arena.add(&plan->d_crc_work, t.crc_work.data(), t.crc_work.size() * sizeof(CrcWork));
  arena.add(&plan->d_scr_work, t.scr_work.data(), t.scr_work.size() * sizeof(ScrWork));
  arena.add(&plan->d_pdus, plan->pdus.data(), plan->pdus.size() * sizeof(PduDev));
  arena.add(&plan->d_work, t.work.data(), t.work.size() * sizeof(CbWork));
  arena.add(&plan->d_dmrs, t.dmrs.data(), t.dmrs.size() * sizeof(DmrsWork));
  arena.add(&plan->d_weights, t.weights.data(), t.weights.size() * sizeof(float));
  arena.add(&plan->d_re_table, t.re_table.data(), t.re_table.size() * sizeof(uint16_t));
  arena.add(&plan->d_zero_work, t.zero_work.data(), t.zero_work.size() * sizeof(ZeroWork));
  arena.add(&plan->d_zero_segs, t.zero_segs.data(), t.zero_segs.size() * sizeof(ZeroSeg));
  void* scratch = nullptr;
  // Behind the tables: what every run rewrites before it reads it -- the sequences and the TB-CRC shares.
  const uint64_t scr_alloc = (std::max<uint64_t>(4, plan->scr_words) + 3U) & ~3ULL;
  const uint64_t scratch_words = scr_alloc + std::max<size_t>(4, t.crc_work.size());
  if (place != nullptr) {
    // Caller-owned memory: no allocation, no copy, no synchronisation here (the asynchronous queue's submit path).
    if (arena.bytes() > place->table_capacity || scratch_words > place->scratch_capacity_words) {
      return NRPHY_ERR_CAPACITY;
    }
    arena.place(place->h_tables, place->d_tables);
    place->table_bytes = arena.bytes();
    scratch            = place->d_scratch;
  } else {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(arena.commit(&plan->d_arena, sizeof(uint32_t) * scratch_words, &scratch));
    // A batch that mixes modulations and is big enough for one launch per bucket (launch_codeblocks) runs those launches side by
    // side: its side streams exist from here on, so that a run makes no HIP object and can be captured in a graph.
    if (!plan_side_streams(plan.get(), side_streams_wanted(plan.get(), 0))) {
      return NRPHY_ERR_DEVICE;
    }
  }
  plan->d_scr    = (uint32_t*)scratch;
  plan->d_tb_crc = plan->d_scr + scr_alloc;
  *out           = plan.release();
  return NRPHY_OK;
}

} // namespace

int nrphy_pdsch_plan_create_placed(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus, const uint64_t* tb_offset,
                                   const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                   uint32_t grid_nof_subc, PlanPlacement* place, nrphy_pdsch_plan_t** out)
{
  return plan_create(ctx, n_pdu, pdus, tb_offset, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, nullptr, out, place);
}

extern "C" int nrphy_pdsch_plan_create(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                                       const uint64_t* tb_offset, const uint32_t* grid_index, uint32_t nof_grids,
                                       uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_pdsch_plan_t** out)
{
  return plan_create(ctx, n_pdu, pdus, tb_offset, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, nullptr, out);
}

extern "C" int nrphy_pdsch_plan_destroy(nrphy_pdsch_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  if (!plan->arena_external) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena); // null for a plan whose creation failed half-way
  }
  for (uint32_t k = 0; k != plan->n_aux; ++k) {
    (void)hipStreamDestroy(plan->aux_stream[k]);
    (void)hipEventDestroy(plan->join_event[k]);
  }
  if (plan->fork_event != nullptr) {
    (void)hipEventDestroy(plan->fork_event);
  }
  for (hipEvent_t e : plan->events) {
    (void)hipEventDestroy(e);
  }
  delete plan;
  return NRPHY_OK;
}

extern "C" uint32_t nrphy_pdsch_plan_nof_codeblocks(const nrphy_pdsch_plan_t* plan)
{
  return plan ? plan->n_cb : 0;
}

extern "C" int nrphy_pdsch_plan_nof_sequences(const nrphy_pdsch_plan_t* plan, uint32_t* scrambling, uint32_t* dmrs)
{
  if (plan == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (scrambling != nullptr) {
    *scrambling = plan->n_scr_seq;
  }
  if (dmrs != nullptr) {
    *dmrs = plan->n_dmrs_seq;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_plan_scrambling_form(const nrphy_pdsch_plan_t* plan)
{
  return plan == nullptr ? -1 : (plan->scr_as_words ? 1 : 0);
}

// The decision launch_codeblocks takes in a run of the plan, from the same rule and the same inputs.
extern "C" int nrphy_pdsch_plan_codeblock_dispatch(const nrphy_pdsch_plan_t* plan)
{
  if (plan == nullptr) {
    return -1;
  }
  PdschLaunch p;
  p.n_work             = plan->n_work;
  uint32_t nof_buckets = 0;
  return codeblocks_take_bucket_launches(p, plan->bucket_begin, plan->ctx->tune.cb_dispatch, &nof_buckets) ? 2 : 1;
}

extern "C" uint64_t nrphy_pdsch_plan_codeword_bits(const nrphy_pdsch_plan_t* plan)
{
  return plan ? plan->cw_bits : 0;
}

extern "C" uint64_t nrphy_pdsch_plan_codeword_offset(const nrphy_pdsch_plan_t* plan, uint32_t pdu)
{
  return (plan && pdu < plan->cw_offset.size()) ? plan->cw_offset[pdu] : 0;
}

extern "C" int nrphy_pdsch_run(nrphy_pdsch_plan_t* plan, const uint8_t* d_tb, void* d_grid, uint8_t* d_cw_rm,
                               uint8_t* d_cw_scrambled, int zero_grids, void* stream)
{
  if (plan == nullptr || d_tb == nullptr || (plan->encode_only && d_grid != nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const TraceRange trace_run("process_pdsch");
  nrphy_ctx*  ctx = plan->ctx;
  hipStream_t s   = stream ? (hipStream_t)stream : ctx->stream;
  PdschLaunch p;
  p.pdus           = plan->d_pdus;
  p.work           = plan->d_work;
  p.dmrs_work      = plan->d_dmrs;
  p.crc_work       = plan->d_crc_work;
  p.scr_work       = plan->d_scr_work;
  p.n_scr_work     = plan->n_scr_work;
  p.tbcrc          = ctx->d_tbcrc;
  p.n_crc_work     = plan->n_crc_work;
  p.weights        = plan->d_weights;
  p.re_table       = plan->d_re_table;
  p.graphs         = ctx->d_graphs;
  p.gold           = ctx->d_gold;
  p.x1_words       = ctx->d_x1;
  p.tb_crc_part        = plan->d_tb_crc;
  const bool merge_dmrs = d_grid != nullptr && !plan->dmrs_separate;
  p.zero_work          = plan->d_zero_work;
  p.zero_segs          = plan->d_zero_segs;
  p.scr                = plan->d_scr;
  p.scr_seq            = plan->d_scr + plan->seed_offset;
  p.scr_as_words       = plan->scr_as_words ? 1U : 0U;
  p.n_zero_work        = (d_grid != nullptr && zero_grids) ? plan->n_zero_work : 0;
  p.zero_fill          = (d_grid != nullptr && zero_grids) ? 1U : 0U;
  p.n_dmrs_in_launch   = merge_dmrs ? plan->n_dmrs : 0;
  p.n_pdu          = (uint32_t)plan->pdus.size();
  p.n_work         = plan->n_work;
  p.work_base      = 0;
  p.n_dmrs_work    = plan->n_dmrs;
  p.grid_nof_ports = plan->grid_nof_ports;
  p.grid_nof_subc  = plan->grid_nof_subc;
  p.lds_lin_words  = plan->lds_lin_words;
  p.lds_u_words    = plan->lds_u_words;
#ifdef NRPHY_PROBES
  // Profiling variant: stop the codeblock waves after a stage to time the stages apart (outputs are then incomplete).
  p.profile_stage = ctx->tune.profile_stage;
#else
  p.profile_stage = 0;
#endif
  const size_t cw_bytes = (size_t)(plan->cw_bits / 8);
  if (d_cw_rm) {
    HIP_TRY(hipMemsetAsync(d_cw_rm, 0, cw_bytes, s));
  }
  if (d_cw_scrambled) {
    HIP_TRY(hipMemsetAsync(d_cw_scrambled, 0, cw_bytes, s));
  }
  hipEvent_t* ev = nullptr;
  if (plan->timed_runs < plan->max_timed_runs && plan->timing_counter++ % plan->timing_stride == 0) {
    ev = &plan->events[4 * plan->timed_runs++];
    HIP_TRY(hipEventRecord(ev[0], s));
  }
  HIP_TRY(launch_prologue(p, d_tb, s));
  if (ev) {
    HIP_TRY(hipEventRecord(ev[1], s));
  }
  {
    const TraceRange trace_cb("CB batch");
    // NRPHY_CB_DISPATCH: 1 = the one-launch mixed kernel, 2 = one launch per (Qm, layers) bucket, unset = by plan shape.
    const int   dispatch     = ctx->tune.cb_dispatch;
    hipStream_t streams[1 + nrphy_pdsch_plan::MAX_AUX] = {s};
    uint32_t    n_streams = 1;
    if (const uint32_t want = side_streams_wanted(plan, dispatch)) {
      // (made at plan creation for a plan that takes bucket launches by its shape; here only when NRPHY_CB_DISPATCH forces
      // them on a small one -- such a first run creates streams and is not for graph capture)
      if (!plan_side_streams(plan, want)) {
        return NRPHY_ERR_DEVICE;
      }
      HIP_TRY(hipEventRecord(plan->fork_event, s));
      for (uint32_t k = 0; k != want; ++k) {
        HIP_TRY(hipStreamWaitEvent(plan->aux_stream[k], plan->fork_event, 0));
        streams[n_streams++] = plan->aux_stream[k];
      }
    }
    HIP_TRY(launch_codeblocks(p, plan->bucket_begin, dispatch, d_tb, (uint32_t*)d_grid, (uint32_t*)d_cw_rm,
                              (uint32_t*)d_cw_scrambled, streams, n_streams));
    for (uint32_t k = 1; k < n_streams; ++k) {
      HIP_TRY(hipEventRecord(plan->join_event[k - 1], streams[k]));
      HIP_TRY(hipStreamWaitEvent(s, plan->join_event[k - 1], 0));
    }
  }
  if (ev) {
    HIP_TRY(hipEventRecord(ev[2], s));
  }
  if (d_grid && !merge_dmrs) {
    // After the data: when data RE share a CDM group with DM-RS the reference lets DM-RS overwrite them.
    const TraceRange trace_dmrs("process_dmrs");
    HIP_TRY(launch_dmrs(p, (uint32_t*)d_grid, s));
    if (ev) {
      HIP_TRY(hipEventRecord(ev[3], s));
    }
  }
  if (ev) { // (an event between two launches costs the stream a few microseconds: none where no launch follows)
    plan->timed_dmrs[plan->timed_runs - 1] = (d_grid && !merge_dmrs) ? 1 : 0;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_plan_enable_timing(nrphy_pdsch_plan_t* plan, uint32_t max_runs)
{
  if (plan == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (hipEvent_t e : plan->events) {
    (void)hipEventDestroy(e);
  }
  plan->events.assign(4 * (size_t)max_runs, nullptr);
  for (hipEvent_t& e : plan->events) {
    HIP_TRY(hipEventCreate(&e));
  }
  plan->timed_dmrs.assign(max_runs, 0);
  plan->max_timed_runs = max_runs;
  plan->timed_runs     = 0;
  plan->timing_counter = 0;
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_plan_timing_stride(nrphy_pdsch_plan_t* plan, uint32_t stride)
{
  if (plan == nullptr || stride == 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  plan->timing_stride  = stride;
  plan->timing_counter = 0;
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_plan_kernel_times(nrphy_pdsch_plan_t* plan, float avg_ms[4], uint32_t* nof_runs)
{
  if (plan == nullptr || avg_ms == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  double sum[4] = {0, 0, 0, 0};
  for (uint32_t r = 0; r != plan->timed_runs; ++r) {
    hipEvent_t*    ev   = &plan->events[4 * r];
    const unsigned last = plan->timed_dmrs[r] ? 3 : 2;
    HIP_TRY(hipEventSynchronize(ev[last]));
    float ms = 0;
    for (unsigned k = 0; k != last; ++k) {
      HIP_TRY(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      sum[k] += ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[last]));
    sum[3] += ms;
  }
  for (int k = 0; k != 4; ++k) {
    avg_ms[k] = plan->timed_runs ? (float)(sum[k] / plan->timed_runs) : 0.f;
  }
  if (nof_runs) {
    *nof_runs = plan->timed_runs;
  }
  plan->timed_runs = 0;
  return NRPHY_OK;
}

// The host-span forms below own their plan through a PlanHandle declared before the HostCall: on every return, HIP_TRY's
// included, the stream is drained first and the plan that its launches read is destroyed after.

extern "C" int nrphy_pdsch_process_host(nrphy_ctx_t* ctx, const nrphy_pdsch_pdu_t* pdu, const uint8_t* tb, void* grid,
                                        uint32_t grid_nof_ports, uint32_t grid_nof_subc, uint8_t* cw_rm,
                                        uint8_t* cw_scrambled)
{
  if (ctx == nullptr || pdu == nullptr || tb == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  PlanHandle          plan;
  HostCall            call(ctx);
  nrphy_pdsch_plan_t* created = nullptr;
  const uint64_t      tb_off  = 0;
  const uint32_t      gi      = 0;
  int rc = nrphy_pdsch_plan_create(ctx, 1, pdu, &tb_off, &gi, 1, grid_nof_ports, grid_nof_subc, &created);
  if (rc != NRPHY_OK) {
    return rc;
  }
  plan.reset(created);
  const size_t tb_alloc   = ((size_t)pdu->tb_size_bytes + 7) & ~(size_t)3;
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t cw_bytes   = (size_t)(plan->cw_bits / 8);
  uint8_t* d_tb   = call.mem<uint8_t>(SCRATCH_TB, tb_alloc);
  uint8_t* d_grid = grid ? call.mem<uint8_t>(SCRATCH_GRID, grid_bytes) : nullptr;
  uint8_t* d_rm   = cw_rm ? call.mem<uint8_t>(SCRATCH_CW_RM, cw_bytes) : nullptr;
  uint8_t* d_scr  = cw_scrambled ? call.mem<uint8_t>(SCRATCH_CW_SCR, cw_bytes) : nullptr;
  if (d_tb == nullptr || (grid && d_grid == nullptr) || (cw_rm && d_rm == nullptr) || (cw_scrambled && d_scr == nullptr)) {
    return NRPHY_ERR_DEVICE;
  }
  // The transport block is readable to the next multiple of 4: clear the tail word, then the bytes.
  HIP_TRY(hipMemsetAsync(d_tb + (tb_alloc - 8), 0, 8, ctx->stream));
  HIP_TRY(hipMemcpyAsync(d_tb, tb, pdu->tb_size_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (grid) {
    HIP_TRY(hipMemcpyAsync(d_grid, grid, grid_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = nrphy_pdsch_run(plan.get(), d_tb, d_grid, d_rm, d_scr, 0, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  nrphy_pdsch_derived_t d;
  nrphy_pdsch_derive(pdu, &d);
  const size_t cw_out = (d.codeword_bits + 7) / 8;
  if (grid) {
    HIP_TRY(hipMemcpyAsync(grid, d_grid, grid_bytes, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (cw_rm) {
    HIP_TRY(hipMemcpyAsync(cw_rm, d_rm, cw_out, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (cw_scrambled) {
    HIP_TRY(hipMemcpyAsync(cw_scrambled, d_scr, cw_out, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_process_slot_host(nrphy_ctx_t* ctx, uint32_t n_pdu, const nrphy_pdsch_pdu_t* pdus,
                                             const uint8_t* const* tbs, void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  if (ctx == nullptr || grid == nullptr || (n_pdu != 0 && (pdus == nullptr || tbs == nullptr))) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (n_pdu == 0) {
    return NRPHY_OK;
  }
  // One plan for the slot: every PDU's codeblocks in one launch, all into grid 0.
  std::vector<uint64_t> tb_off(n_pdu);
  std::vector<uint32_t> grid_of(n_pdu, 0);
  size_t                tb_total = 0;
  for (uint32_t i = 0; i != n_pdu; ++i) {
    if (tbs[i] == nullptr) {
      return NRPHY_ERR_ARGUMENT;
    }
    tb_off[i] = tb_total;
    tb_total += ((size_t)pdus[i].tb_size_bytes + 7) & ~(size_t)3; // readable to the next multiple of 4
  }
  PlanHandle          plan;
  HostCall            call(ctx);
  nrphy_pdsch_plan_t* created = nullptr;
  int rc = nrphy_pdsch_plan_create(ctx, n_pdu, pdus, tb_off.data(), grid_of.data(), 1, grid_nof_ports, grid_nof_subc, &created);
  if (rc != NRPHY_OK) {
    return rc;
  }
  plan.reset(created);
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  uint8_t* d_tb   = call.mem<uint8_t>(SCRATCH_TB, tb_total + 8);
  uint8_t* d_grid = call.mem<uint8_t>(SCRATCH_GRID, grid_bytes);
  if (d_tb == nullptr || d_grid == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemsetAsync(d_tb, 0, tb_total + 8, ctx->stream));
  for (uint32_t i = 0; i != n_pdu; ++i) {
    HIP_TRY(hipMemcpyAsync(d_tb + tb_off[i], tbs[i], pdus[i].tb_size_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(hipMemcpyAsync(d_grid, grid, grid_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = nrphy_pdsch_run(plan.get(), d_tb, d_grid, nullptr, nullptr, 0, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(grid, d_grid, grid_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  return NRPHY_OK;
}

extern "C" int nrphy_pdsch_encode_host(nrphy_ctx_t* ctx, const nrphy_pdsch_encoder_cfg_t* cfg, const uint8_t* tb,
                                       uint8_t* codeword_bits, uint8_t* codeword_packed)
{
  if (ctx == nullptr || cfg == nullptr || tb == nullptr || cfg->nof_layers == 0 ||
      cfg->nof_ch_symbols % cfg->nof_layers != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_pdsch_pdu_t pdu;
  std::memset(&pdu, 0, sizeof(pdu));
  pdu.qm              = cfg->qm;
  pdu.rv              = cfg->rv;
  pdu.nof_codewords   = 1;
  pdu.ldpc_base_graph = cfg->base_graph;
  pdu.tb_size_bytes   = cfg->tb_size_bytes;
  pdu.nof_layers      = cfg->nof_layers;
  pdu.nof_ports       = 1;
  pdu.nof_prg         = 1;
  pdu.prg_size_rb     = NRPHY_MAX_RB;
  pdu.tbs_lbrm_bytes  = 1; // unused: N_ref is given
  const EncodeOnly    enc    = {cfg->nof_ch_symbols / cfg->nof_layers, cfg->nref};
  std::vector<uint8_t> packed_local; // a copy target: declared before `call`, so that it outlives the drain
  PlanHandle           plan;
  HostCall             call(ctx);
  nrphy_pdsch_plan_t* created = nullptr;
  const uint64_t      tb_off  = 0;
  const uint32_t      gi      = 0;
  int                 rc      = plan_create(ctx, 1, &pdu, &tb_off, &gi, 1, 1, 12, &enc, &created);
  if (rc != NRPHY_OK) {
    return rc;
  }
  plan.reset(created);
  const size_t cw_bits  = (size_t)cfg->nof_ch_symbols * cfg->qm;
  const size_t cw_bytes = (size_t)(plan->cw_bits / 8);
  const size_t tb_alloc = ((size_t)cfg->tb_size_bytes + 7) & ~(size_t)3;
  uint8_t*     packed   = codeword_packed;
  if (packed == nullptr) {
    packed_local.resize((cw_bits + 7) / 8);
    packed = packed_local.data();
  }
  uint8_t* d_tb = call.mem<uint8_t>(SCRATCH_TB, tb_alloc);
  uint8_t* d_rm = call.mem<uint8_t>(SCRATCH_CW_RM, cw_bytes);
  if (d_tb == nullptr || d_rm == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemsetAsync(d_tb + (tb_alloc - 8), 0, 8, ctx->stream));
  HIP_TRY(hipMemcpyAsync(d_tb, tb, cfg->tb_size_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = nrphy_pdsch_run(plan.get(), d_tb, nullptr, d_rm, nullptr, 0, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(packed, d_rm, (cw_bits + 7) / 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(call.sync());
  if (codeword_bits != nullptr) { // the reference's codeword span: one bit per byte
    for (size_t i = 0; i != cw_bits; ++i) {
      codeword_bits[i] = (packed[i >> 3] >> (7U - (i & 7U))) & 1U;
    }
  }
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_encode(nrphy_ctx_t* ctx, uint32_t base_graph, uint32_t lifting_size, uint32_t n_cb,
                                 const uint8_t* d_msg, uint32_t msg_stride_bytes, uint32_t out_bits, uint8_t* d_out,
                                 uint32_t out_stride_bytes, void* stream)
{
  if (ctx == nullptr || (base_graph != 1 && base_graph != 2) || d_msg == nullptr || d_out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const int pos = lifting_position(lifting_size);
  const unsigned kb = (base_graph == 1) ? 22 : 10, nfull = (base_graph == 1) ? 68 : 52;
  if (pos < 0 || out_bits == 0 || out_bits > (nfull - 2) * lifting_size ||
      msg_stride_bytes < (kb * lifting_size + 7) / 8 || out_stride_bytes < (out_bits + 7) / 8) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(launch_ldpc_encode(ctx->d_graphs, (base_graph - 1) * NOF_LIFTING_SIZES + (uint32_t)pos, kb, lifting_size,
                             n_cb, d_msg, msg_stride_bytes, out_bits, d_out, out_stride_bytes,
                             stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}
