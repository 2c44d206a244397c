// Host side of the UL-SCH demultiplexer (ulsch_kernels.hip): validation, sizes, and per codeword of a plan the placement table
// of ulsch_placement_host.h with the codeword's descriptor.
#include "pusch_select_host.h"
#include "ulsch_placement_host.h"

namespace {

uint32_t alignment_unit(uint64_t v) // 16, 4 or 1: the largest copy unit that divides v
{
  return v % 16 == 0 ? 16 : v % 4 == 0 ? 4 : 1;
}

} // namespace

struct nrphy_ulsch_demux_plan {
  nrphy_ctx*       ctx       = nullptr;
  void*            d_arena   = nullptr;
  UlschCwDesc*     d_cw      = nullptr;
  uint32_t*        d_block   = nullptr;
  uint32_t*        d_map     = nullptr;
  UlschSpecialDev* d_special = nullptr;
  uint32_t         nof_blocks = 0;
  bool             uses[4]    = {true, false, false, false}; // streams some codeword writes
  bool             selects    = false;                       // some codeword names a select word
};

extern "C" int nrphy_ulsch_demux_validate(const nrphy_ulsch_demux_cfg_t* cfg)
{
  UlschPlacement p;
  return cfg != nullptr && ulsch_placement(*cfg, p) ? NRPHY_OK : NRPHY_ERR_ARGUMENT;
}

extern "C" int nrphy_ulsch_demux_sizes(const nrphy_ulsch_demux_cfg_t* cfg, nrphy_ulsch_demux_sizes_t* sizes)
{
  UlschPlacement p;
  if (cfg == nullptr || sizes == nullptr || !ulsch_placement(*cfg, p)) {
    return NRPHY_ERR_ARGUMENT;
  }
  sizes->nof_sch_bits      = p.nof_re[ULSCH_SCH] * p.bits_per_re;
  sizes->nof_codeword_bits = (uint32_t)p.map.size() * p.bits_per_re;
  return NRPHY_OK;
}

extern "C" int nrphy_ulsch_demux_plan_destroy(nrphy_ulsch_demux_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  if (plan->d_arena != nullptr) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena);
  }
  delete plan;
  return NRPHY_OK;
}

int ulsch_demux_plan_create_select(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ulsch_demux_cfg_t* cfgs, const uint64_t* in_offset,
                                   const uint64_t* sch_offset, const uint64_t* harq_offset, const uint64_t* csi1_offset,
                                   const uint64_t* csi2_offset, const uint32_t* select_word, const uint32_t* select_value,
                                   nrphy_ulsch_demux_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || cfgs == nullptr || in_offset == nullptr || sch_offset == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint64_t*              offsets[4] = {sch_offset, harq_offset, csi1_offset, csi2_offset};
  std::vector<UlschCwDesc>     cw(n);
  std::vector<uint32_t>        block_cw, map;
  std::vector<UlschSpecialDev> special;
  auto*                        plan = new nrphy_ulsch_demux_plan;
  plan->ctx                         = ctx;
  UlschPlacement p;
  for (uint32_t i = 0; i != n; ++i) {
    const nrphy_ulsch_demux_cfg_t& c = cfgs[i];
    if (!ulsch_placement(c, p) || c.rnti > 0xFFFF || c.n_id > 1023) {
      delete plan;
      return NRPHY_ERR_ARGUMENT;
    }
    UlschCwDesc& d = cw[i];
    std::memset(&d, 0, sizeof(d));
    d.in_offset   = in_offset[i];
    d.nof_re      = (uint32_t)p.map.size();
    d.bits_per_re = p.bits_per_re;
    ulsch_bits_per_symbol(c.modulation, &d.qm);
    d.unit = alignment_unit(p.bits_per_re | d.in_offset);
    for (uint32_t s = 0; s != 4; ++s) {
      if (p.nof_re[s] == 0) {
        continue;
      }
      if (offsets[s] == nullptr) { // a stream this codeword writes has no place
        delete plan;
        return NRPHY_ERR_ARGUMENT;
      }
      plan->uses[s]   = true;
      d.out_offset[s] = offsets[s][i];
      d.unit          = std::min(d.unit, alignment_unit(d.out_offset[s]));
    }
    d.map_offset     = (uint32_t)map.size();
    d.special_offset = (uint32_t)special.size();
    d.nof_special    = (uint32_t)p.special.size();
    d.c_init         = c.rnti * (1U << 15) + c.n_id;
    d.select_word    = select_word != nullptr && select_value != nullptr ? select_word[i] : NO_SELECT_WORD;
    d.select_value   = d.select_word != NO_SELECT_WORD ? select_value[i] : 0;
    plan->selects    = plan->selects || d.select_word != NO_SELECT_WORD;
    map.insert(map.end(), p.map.begin(), p.map.end());
    for (const UlschSpecial& s : p.special) {
      special.push_back({s.src, s.dst, s.stream, s.fix});
    }
    const uint32_t per_block = ULSCH_THREADS * ULSCH_UNITS_PER_THREAD;
    const uint32_t units     = d.nof_re * (d.bits_per_re / d.unit);
    d.first_block            = (uint32_t)block_cw.size();
    d.nof_copy_blocks        = (units + per_block - 1) / per_block;
    const uint32_t items     = d.nof_special * c.nof_layers;
    block_cw.insert(block_cw.end(), d.nof_copy_blocks + (items + ULSCH_THREADS - 1) / ULSCH_THREADS, i);
  }
  plan->nof_blocks = (uint32_t)block_cw.size();
  DeviceArena arena;
  arena.add(&plan->d_cw, cw.data(), cw.size() * sizeof(UlschCwDesc));
  arena.add(&plan->d_block, block_cw.data(), block_cw.size() * sizeof(uint32_t));
  arena.add(&plan->d_map, map.data(), map.size() * sizeof(uint32_t));
  arena.add(&plan->d_special, special.data(), special.size() * sizeof(UlschSpecialDev));
  void* unused = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || arena.commit(&plan->d_arena, 0, &unused) != hipSuccess) {
    nrphy_ulsch_demux_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  *out = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_ulsch_demux_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_ulsch_demux_cfg_t* cfgs,
                                             const uint64_t* in_offset, const uint64_t* sch_offset, const uint64_t* harq_offset,
                                             const uint64_t* csi1_offset, const uint64_t* csi2_offset,
                                             nrphy_ulsch_demux_plan_t** out)
{
  return ulsch_demux_plan_create_select(ctx, n, cfgs, in_offset, sch_offset, harq_offset, csi1_offset, csi2_offset, nullptr, nullptr,
                                        out);
}

int ulsch_demux_run_select(nrphy_ulsch_demux_plan_t* plan, const int8_t* d_codeword_llr, int8_t* d_sch, int8_t* d_harq_ack,
                           int8_t* d_csi1, int8_t* d_csi2, const uint32_t* d_select, void* stream)
{
  if (plan == nullptr || d_codeword_llr == nullptr || (plan->selects && d_select == nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  UlschLaunch p;
  p.select     = plan->selects ? d_select : nullptr;
  p.cw         = plan->d_cw;
  p.block_cw   = plan->d_block;
  p.map        = plan->d_map;
  p.special    = plan->d_special;
  p.gold       = plan->ctx->d_gold;
  p.x1_words   = plan->ctx->d_x1;
  p.in         = d_codeword_llr;
  p.out[0]     = d_sch;
  p.out[1]     = d_harq_ack;
  p.out[2]     = d_csi1;
  p.out[3]     = d_csi2;
  p.nof_blocks = plan->nof_blocks;
  uintptr_t bits = (uintptr_t)d_codeword_llr;
  for (uint32_t s = 0; s != 4; ++s) {
    if (plan->uses[s]) {
      if (p.out[s] == nullptr) {
        return NRPHY_ERR_ARGUMENT;
      }
      bits |= (uintptr_t)p.out[s];
    }
  }
  p.ptr_unit = alignment_unit(bits & 15U);
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_ulsch_demux(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_ulsch_demux_run(nrphy_ulsch_demux_plan_t* plan, const int8_t* d_codeword_llr, int8_t* d_sch, int8_t* d_harq_ack,
                                     int8_t* d_csi1, int8_t* d_csi2, void* stream)
{
  return ulsch_demux_run_select(plan, d_codeword_llr, d_sch, d_harq_ack, d_csi1, d_csi2, nullptr, stream);
}

extern "C" int nrphy_ulsch_demultiplex_host(nrphy_ctx_t* ctx, const nrphy_ulsch_demux_cfg_t* cfg, const int8_t* codeword_llr,
                                            int8_t* sch, int8_t* harq_ack, int8_t* csi1, int8_t* csi2)
{
  UlschPlacement p;
  if (ctx == nullptr || cfg == nullptr || codeword_llr == nullptr || !ulsch_placement(*cfg, p)) {
    return NRPHY_ERR_ARGUMENT;
  }
  int8_t* host[4] = {sch, harq_ack, csi1, csi2};
  size_t  bytes[5] = {p.map.size() * p.bits_per_re, 0, 0, 0, 0};
  for (uint32_t s = 0; s != 4; ++s) {
    bytes[1 + s] = (size_t)p.nof_re[s] * p.bits_per_re;
    if (bytes[1 + s] != 0 && host[s] == nullptr) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  HostCall call(ctx);
  uint8_t* d[5]; // codeword, then the four streams
  if (!call.carve(SCRATCH_RX, bytes, d)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d[0], codeword_llr, bytes[0], hipMemcpyHostToDevice));
  uint64_t offset[5];
  for (uint32_t k = 0; k != 5; ++k) {
    offset[k] = (uint64_t)(d[k] - d[0]);
  }
  // The plan is made and released inside the call: an allocation and a blocking upload of the placement table per call, the
  // price of the convenience form.
  nrphy_ulsch_demux_plan_t* plan = nullptr;
  int rc = nrphy_ulsch_demux_plan_create(ctx, 1, cfg, &offset[0], &offset[1], &offset[2], &offset[3], &offset[4], &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_ulsch_demux_run(plan, (const int8_t*)d[0], (int8_t*)d[0], (int8_t*)d[0], (int8_t*)d[0], (int8_t*)d[0], ctx->stream);
  if (rc == NRPHY_OK && call.sync() != hipSuccess) {
    rc = NRPHY_ERR_DEVICE;
  }
  for (uint32_t s = 0; rc == NRPHY_OK && s != 4; ++s) {
    if (bytes[1 + s] != 0 && hipMemcpy(host[s], d[1 + s], bytes[1 + s], hipMemcpyDeviceToHost) != hipSuccess) {
      rc = NRPHY_ERR_DEVICE;
    }
  }
  nrphy_ulsch_demux_plan_destroy(plan);
  return rc;
}
