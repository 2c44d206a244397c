// Host side of the PUSCH processor with CSI part 2 (pusch_csi2_kernels.hip): the variant table of a PDU -- every size its part 2
// can take (pusch_csi2_host.h), and for each the UL-SCH information, the demultiplexer, UCI decoder and transport-block decoder
// configurations, derived with the code of the stages -- and the plan that owns a PUSCH processor plan (pusch_proc_host.cpp) for
// the launches up to CSI part 1, plus one demultiplexer plan and one UCI decoder plan that hold every variant of every PDU.
#include "ldpc_receive_host.h"
#include "pusch_csi2_host.h"
#include "pusch_proc_plan_host.h"
#include "pusch_select_host.h"
#include "ulsch_info_host.h"

namespace {

constexpr uint64_t ALIGN = 256;

uint64_t align_up(uint64_t v, uint64_t a = ALIGN)
{
  return (v + a - 1) / a * a;
}

struct Csi2Variants {
  nrphy_pusch_proc_derived_t base; // the PDU without part 2: variant 0
  uint32_t                   n = 0;
  uint32_t                   size[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
  nrphy_ulsch_info_t         info[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
  nrphy_ulsch_demux_cfg_t    demux[NRPHY_PUSCH_CSI2_MAX_VARIANTS];   // rows 1 .. n - 1
  nrphy_uci_decoder_cfg_t    uci[NRPHY_PUSCH_CSI2_MAX_VARIANTS];     // rows 1 .. n - 1: the part 2 message
  nrphy_pusch_decoder_cfg_t  decoder[NRPHY_PUSCH_CSI2_MAX_VARIANTS]; // rows 0 .. n - 1 of a PDU with description
};

int derive_variants(const nrphy_pusch_pdu_t* p, const nrphy_pusch_csi2_desc_t* desc, const nrphy_pusch_proc_options_t* o,
                    uint32_t grid_nof_ports, uint32_t grid_nof_subc, Csi2Variants& out)
{
  if (p == nullptr || desc == nullptr || o == nullptr || p->nof_csi_part2_entries != desc->nof_entries) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_pusch_pdu_t plain = *p;
  plain.nof_csi_part2_entries = 0;
  if (nrphy_pusch_proc_derive(&plain, o, grid_nof_ports, grid_nof_subc, &out.base) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }
  out.n       = 1;
  out.size[0] = 0;
  out.info[0] = out.base.info;
  if (desc->nof_entries == 0) {
    return NRPHY_OK;
  }
  // A PDU without codeword is refused: G^CSI-1 itself depends there on whether part 2 is present (ulsch_info_host.h).
  if (!pusch_csi2_desc_ok(*desc, p->nof_csi_part1) || p->has_codeword == 0 || out.base.has_decoder == 0 ||
      !pusch_csi2_enumerate(*desc, &out.n, out.size)) {
    return NRPHY_ERR_ARGUMENT;
  }
  out.decoder[0] = out.base.decoder;
  uint64_t soft0 = 0, state0 = 0;
  uint32_t ncb0 = 0;
  if (!pusch_decoder_harq_sizes(out.decoder[0], 1, &soft0, &state0, &ncb0)) {
    return NRPHY_ERR_ARGUMENT;
  }
  for (uint32_t v = 1; v != out.n; ++v) {
    const nrphy_ulsch_info_cfg_t ic   = pusch_proc_info_cfg(*p, out.base.demux.nof_prb, out.size[v]);
    nrphy_ulsch_info_t&          info = out.info[v];
    // With UL-SCH neither G^ACK nor G^CSI-1 depends on part 2: the streams variant 0 left behind stay what they are.
    if (ulsch_info(ic, info) != NRPHY_OK || info.nof_csi_part2_bits == 0 || info.nof_harq_ack_bits != out.base.info.nof_harq_ack_bits ||
        info.nof_harq_ack_rvd != out.base.info.nof_harq_ack_rvd || info.nof_csi_part1_bits != out.base.info.nof_csi_part1_bits) {
      return NRPHY_ERR_ARGUMENT;
    }
    nrphy_ulsch_demux_cfg_t& dx = out.demux[v];
    dx                          = out.base.demux;
    dx.nof_csi_part2_bits       = out.size[v];
    dx.nof_enc_csi_part2_bits   = info.nof_csi_part2_bits;
    nrphy_ulsch_demux_sizes_t sizes;
    if (nrphy_ulsch_demux_sizes(&dx, &sizes) != NRPHY_OK || sizes.nof_codeword_bits != out.base.codeword_bits ||
        sizes.nof_sch_bits != info.nof_ul_sch_bits || sizes.nof_sch_bits == 0 || sizes.nof_sch_bits > out.base.nof_sch_bits) {
      return NRPHY_ERR_ARGUMENT;
    }
    out.uci[v] = {out.size[v], info.nof_csi_part2_bits, p->modulation, 0};
    if (nrphy_uci_decoder_validate(&out.uci[v]) != NRPHY_OK) {
      return NRPHY_ERR_ARGUMENT;
    }
    nrphy_pusch_decoder_cfg_t& dc = out.decoder[v];
    dc                            = out.base.decoder;
    dc.nof_ch_symbols             = sizes.nof_sch_bits / dc.qm;
    uint64_t soft = 0, state = 0;
    uint32_t ncb = 0;
    if (!pusch_decoder_harq_sizes(dc, 1, &soft, &state, &ncb) || soft != soft0 || state != state0 || ncb != ncb0) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  return NRPHY_OK;
}

uint32_t largest_size(const Csi2Variants& v)
{
  return v.size[v.n - 1]; // ascending
}

} // namespace

struct nrphy_pusch_csi2_plan {
  nrphy_ctx*                ctx   = nullptr;
  uint32_t                  n     = 0;
  nrphy_pusch_proc_plan_t*  base  = nullptr;
  nrphy_ulsch_demux_plan_t* demux = nullptr; // every (PDU, variant > 0) as a codeword
  nrphy_uci_decoder_plan_t* uci   = nullptr; // every (PDU, variant > 0) as a message
  // per decoder of the base plan: the decoder configurations of the PDU's variants, empty for a PDU without description
  std::vector<std::vector<nrphy_pusch_decoder_cfg_t>> variant_cfg;
  void*          d_arena    = nullptr;
  PuschCsi2Desc* d_desc     = nullptr;
  uint32_t*      d_select   = nullptr;
  uint32_t*      d_status   = nullptr;
  int8_t*        d_csi2_llr = nullptr;
  int8_t*        d_dump     = nullptr; // where the variants' codewords write the HARQ-ACK and CSI part 1 streams a second time
};

extern "C" int nrphy_pusch_csi2_size(const nrphy_pusch_csi2_desc_t* desc, const uint8_t* csi_part1_bits, uint32_t nof_csi_part1,
                                     uint32_t* size)
{
  if (desc == nullptr || csi_part1_bits == nullptr || size == nullptr || !pusch_csi2_desc_ok(*desc, nof_csi_part1)) {
    return NRPHY_ERR_ARGUMENT;
  }
  *size = pusch_csi2_size(*desc, csi_part1_bits);
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_csi2_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                                         const nrphy_pusch_proc_options_t* options, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  Csi2Variants v;
  return derive_variants(pdu, desc, options, grid_nof_ports, grid_nof_subc, v);
}

extern "C" int nrphy_pusch_csi2_variants(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                                         const nrphy_pusch_proc_options_t* options, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                         uint32_t* nof_variants, uint32_t* sizes, nrphy_ulsch_info_t* infos)
{
  if (nof_variants == nullptr || sizes == nullptr || infos == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *nof_variants = 0;
  Csi2Variants v;
  const int    rc = derive_variants(pdu, desc, options, grid_nof_ports, grid_nof_subc, v);
  if (rc != NRPHY_OK) {
    return rc;
  }
  *nof_variants = v.n;
  std::copy(v.size, v.size + v.n, sizes);
  std::copy(v.info, v.info + v.n, infos);
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_csi2_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                                           const nrphy_pusch_proc_options_t* options, uint64_t* soft_bytes, uint64_t* state_bytes)
{
  if (pdu == nullptr || desc == nullptr || pdu->nof_csi_part2_entries != desc->nof_entries) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_pusch_pdu_t plain = *pdu;
  plain.nof_csi_part2_entries = 0;
  return nrphy_pusch_proc_harq_bytes(&plain, options, soft_bytes, state_bytes);
}

extern "C" int nrphy_pusch_csi2_plan_destroy(nrphy_pusch_csi2_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  nrphy_pusch_proc_plan_destroy(plan->base);
  nrphy_ulsch_demux_plan_destroy(plan->demux);
  nrphy_uci_decoder_plan_destroy(plan->uci);
  if (plan->d_arena != nullptr) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena);
  }
  delete plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_csi2_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                            const nrphy_pusch_csi2_desc_t* descs, const nrphy_pusch_proc_options_t* options,
                                            const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                                            uint32_t grid_nof_subc, const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset,
                                            const uint64_t* tb_offset, const uint64_t* uci_offset, const uint64_t* csi2_offset,
                                            nrphy_pusch_csi2_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || n > 65535U || pdus == nullptr || descs == nullptr || options == nullptr || grid_index == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<Csi2Variants>      variants(n);
  std::vector<nrphy_pusch_pdu_t> plain(pdus, pdus + n);
  for (uint32_t i = 0; i != n; ++i) {
    if (derive_variants(&pdus[i], &descs[i], options, grid_nof_ports, grid_nof_subc, variants[i]) != NRPHY_OK ||
        (variants[i].n > 1 && csi2_offset == nullptr)) {
      return NRPHY_ERR_ARGUMENT;
    }
    plain[i].nof_csi_part2_entries = 0;
  }
  auto* plan = new nrphy_pusch_csi2_plan;
  plan->ctx  = ctx;
  plan->n    = n;
  int rc = nrphy_pusch_proc_plan_create(ctx, n, plain.data(), options, grid_index, nof_grids, grid_nof_ports, grid_nof_subc,
                                        harq_soft_offset, harq_state_offset, tb_offset, uci_offset, &plan->base);
  if (rc != NRPHY_OK) {
    nrphy_pusch_csi2_plan_destroy(plan);
    return rc;
  }
  const nrphy_pusch_proc_plan_t& base = *plan->base;
  std::vector<PuschCsi2Desc>           desc(n);
  std::vector<nrphy_ulsch_demux_cfg_t> demux;
  std::vector<uint64_t>                dx_in, dx_sch, dx_harq, dx_csi1, dx_csi2;
  std::vector<nrphy_uci_decoder_cfg_t> uci;
  std::vector<uint64_t>                uci_llr, uci_msg;
  std::vector<uint32_t>                select_word, select_value;
  uint64_t                             csi2_llr_bytes = 0, dump_bytes = 0;
  plan->variant_cfg.resize(base.decoders.size());
  for (size_t k = 0; k != base.decoders.size(); ++k) {
    const ProcDecoder&  dec = base.decoders[k];
    const Csi2Variants& v   = variants[dec.pdu];
    if (v.n > 1) {
      plan->variant_cfg[k].assign(v.decoder, v.decoder + v.n);
    }
  }
  for (uint32_t i = 0; i != n; ++i) {
    const Csi2Variants& v = variants[i];
    PuschCsi2Desc&      d = desc[i];
    std::memset(&d, 0, sizeof(d));
    d.nof_entries  = descs[i].nof_entries;
    d.nof_variants = v.n;
    d.csi1_status  = base.desc[i].csi1_status;
    d.status_base  = (uint32_t)uci.size();
    d.csi1_offset  = base.desc[i].csi_part1_offset;
    d.csi2_offset  = v.n > 1 ? csi2_offset[i] : 0;
    for (uint32_t e = 0; e != descs[i].nof_entries; ++e) {
      const nrphy_pusch_csi2_entry_t& entry = descs[i].entries[e];
      d.nof_parameters[e]                   = entry.nof_parameters;
      for (uint32_t k = 0; k != entry.nof_parameters; ++k) {
        d.offset[e][k] = entry.offset[k];
        d.width[e][k]  = entry.width[k];
      }
      std::copy(entry.map, entry.map + entry.map_size, d.map[e]);
    }
    for (uint32_t r = 0; r != v.n; ++r) {
      d.size[r]       = v.size[r];
      d.nof_enc[r]    = v.info[r].nof_csi_part2_bits;
      d.nof_ul_sch[r] = v.info[r].nof_ul_sch_bits;
    }
    if (v.n == 1) {
      continue;
    }
    // The PDU's UL-SCH stream in the base plan's buffer: where its decoder reads (a PDU with description has UCI and a codeword).
    uint64_t sch_at = 0;
    bool     found  = false;
    for (const ProcDecoder& dec : base.decoders) {
      if (dec.pdu == i && dec.from_sch) {
        sch_at = dec.llr_offset;
        found  = true;
      }
    }
    if (!found) { // no UL-SCH stream of the demultiplexer's to rewrite: not a PDU derive_variants accepts
      nrphy_pusch_csi2_plan_destroy(plan);
      return NRPHY_ERR_ARGUMENT;
    }
    const uint64_t harq_at = dump_bytes, csi1_at = harq_at + align_up(v.base.info.nof_harq_ack_bits, 16);
    dump_bytes             = csi1_at + align_up(v.base.info.nof_csi_part1_bits, 16);
    const uint64_t csi2_at   = csi2_llr_bytes;
    uint64_t       csi2_room = 0;
    for (uint32_t r = 1; r != v.n; ++r) { // the variants of a PDU share its part 2 stream: one of them runs
      csi2_room = std::max(csi2_room, align_up(v.info[r].nof_csi_part2_bits, 16));
      demux.push_back(v.demux[r]);
      dx_in.push_back(i * base.llr_stride);
      dx_sch.push_back(sch_at);
      dx_harq.push_back(harq_at);
      dx_csi1.push_back(csi1_at);
      dx_csi2.push_back(csi2_at);
      uci.push_back(v.uci[r]);
      uci_llr.push_back(csi2_at);
      uci_msg.push_back(csi2_offset[i]);
      select_word.push_back(i);
      select_value.push_back(r);
    }
    csi2_llr_bytes = csi2_at + csi2_room;
  }
  if (!demux.empty()) {
    rc = ulsch_demux_plan_create_select(ctx, (uint32_t)demux.size(), demux.data(), dx_in.data(), dx_sch.data(), dx_harq.data(),
                                        dx_csi1.data(), dx_csi2.data(), select_word.data(), select_value.data(), &plan->demux);
    if (rc == NRPHY_OK) {
      rc = uci_decoder_plan_create_select(ctx, (uint32_t)uci.size(), uci.data(), uci_llr.data(), uci_msg.data(), select_word.data(),
                                          select_value.data(), &plan->uci);
    }
    if (rc != NRPHY_OK) {
      nrphy_pusch_csi2_plan_destroy(plan);
      return rc;
    }
  }
  const uint64_t piece[] = {(uint64_t)n * sizeof(uint32_t), (uint64_t)uci.size() * sizeof(uint32_t), csi2_llr_bytes, dump_bytes};
  constexpr size_t NP = sizeof(piece) / sizeof(piece[0]);
  uint64_t         at[NP + 1] = {};
  for (size_t k = 0; k != NP; ++k) {
    at[k + 1] = at[k] + align_up(std::max<uint64_t>(piece[k], 16));
  }
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PuschCsi2Desc));
  uint8_t* ws = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || arena.commit(&plan->d_arena, at[NP], (void**)&ws) != hipSuccess ||
      hipMemset(ws, 0, at[NP]) != hipSuccess) {
    nrphy_pusch_csi2_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  plan->d_select   = (uint32_t*)(ws + at[0]);
  plan->d_status   = (uint32_t*)(ws + at[1]);
  plan->d_csi2_llr = (int8_t*)(ws + at[2]);
  plan->d_dump     = (int8_t*)(ws + at[3]);
  *out             = plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_csi2_run(nrphy_pusch_csi2_plan_t* plan, const void* d_grid, void* d_harq, uint8_t* d_tb, uint8_t* d_uci_bits,
                                    nrphy_pusch_result_t* d_result, nrphy_pusch_csi2_result_t* d_csi2_result, void* stream)
{
  if (plan == nullptr || d_csi2_result == nullptr || ((uintptr_t)d_csi2_result & 7U) != 0 ||
      !pusch_proc_run_arguments_ok(plan->base, d_grid, d_harq, d_tb, d_uci_bits, d_result)) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_pusch_proc_plan_t* base = plan->base;
  hipStream_t              s    = stream ? (hipStream_t)stream : plan->ctx->stream;
  // Estimator, demodulator, demultiplexer without part 2, HARQ-ACK and CSI part 1: variant 0's UL-SCH stream is in place.
  int rc = pusch_proc_run_front(base, d_grid, d_uci_bits, stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  PuschCsi2Launch p;
  p.desc           = plan->d_desc;
  p.status         = base->d_status;
  p.variant_status = plan->d_status;
  p.uci_bits       = d_uci_bits;
  p.select         = plan->d_select;
  p.result         = d_csi2_result;
  p.n              = plan->n;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pusch_csi2_select(p, s));
  if (plan->demux != nullptr) {
    rc = ulsch_demux_run_select(plan->demux, base->d_llr, base->d_sch, plan->d_dump, plan->d_dump, plan->d_csi2_llr, plan->d_select,
                                stream);
    if (rc == NRPHY_OK) {
      rc = uci_decoder_run_select(plan->uci, plan->d_csi2_llr, d_uci_bits, plan->d_status, plan->d_select, stream);
    }
  }
  for (size_t k = 0; k != base->decoders.size() && rc == NRPHY_OK; ++k) {
    const std::vector<nrphy_pusch_decoder_cfg_t>& cfgs = plan->variant_cfg[k];
    if (cfgs.empty()) {
      rc = pusch_proc_run_decoder(base, k, d_harq, d_tb, stream);
      continue;
    }
    const ProcDecoder& dec = base->decoders[k];
    PuschDecodeVariant variants[NRPHY_PUSCH_CSI2_MAX_VARIANTS];
    for (size_t v = 0; v != cfgs.size(); ++v) { // every variant's UL-SCH stream starts where variant 0's does
      variants[v] = {&cfgs[v], base->d_sch + dec.llr_offset, (uint32_t)v};
    }
    rc = pusch_decode_variants(plan->ctx, variants, (uint32_t)cfgs.size(), plan->d_select + dec.pdu, 1,
                               (uint64_t)cfgs[0].nof_ch_symbols * cfgs[0].qm, (int8_t*)d_harq + dec.soft_offset,
                               (uint8_t*)d_harq + dec.state_offset, base->d_scratch, d_tb + dec.tb_offset, dec.cfg.tb_size_bytes,
                               base->d_dec + 4 * (size_t)dec.pdu, stream);
  }
  if (rc == NRPHY_OK) {
    rc = pusch_proc_run_result(base, d_result, stream);
  }
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(launch_pusch_csi2_result(p, s));
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_csi2_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_csi2_desc_t* desc,
                                     const nrphy_pusch_proc_options_t* options, const void* grid, uint32_t grid_nof_ports,
                                     uint32_t grid_nof_subc, int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits,
                                     uint8_t* csi2_bits, nrphy_pusch_result_t* result, nrphy_pusch_csi2_result_t* csi2_result)
{
  if (ctx == nullptr || grid == nullptr || result == nullptr || csi2_result == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  Csi2Variants v;
  int          rc = derive_variants(pdu, desc, options, grid_nof_ports, grid_nof_subc, v);
  if (rc != NRPHY_OK) {
    return rc;
  }
  uint64_t soft_bytes = 0, state_bytes = 0;
  uint32_t ncb = 0;
  const bool has_decoder = v.base.has_decoder != 0;
  if (has_decoder && (harq_soft == nullptr || harq_state == nullptr || tb == nullptr ||
                      !pusch_decoder_harq_sizes(v.base.decoder, 1, &soft_bytes, &state_bytes, &ncb))) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t uci_bytes = pdu->nof_harq_ack + pdu->nof_csi_part1, csi2_bytes = largest_size(v);
  if ((uci_bytes != 0 && uci_bits == nullptr) || (csi2_bytes != 0 && csi2_bits == nullptr)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t soft_room  = align_up(soft_bytes);
  const size_t uci_off = align_up(pdu->tb_size_bytes), csi2_off = uci_off + align_up(uci_bytes);
  HostCall call(ctx);
  uint8_t* dv[4]; // grid, HARQ arena (soft block, then state block), transport block + UCI payloads, the two results
  if (!call.carve(SCRATCH_RX, {grid_bytes, soft_room + (size_t)state_bytes, csi2_off + csi2_bytes,
                               align_up(sizeof(nrphy_pusch_result_t)) + sizeof(nrphy_pusch_csi2_result_t)}, dv)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(dv[0], grid, grid_bytes, hipMemcpyHostToDevice));
  if (has_decoder) {
    HIP_TRY(hipMemcpy(dv[1], harq_soft, soft_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv[1] + soft_room, harq_state, state_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv[2], tb, pdu->tb_size_bytes, hipMemcpyHostToDevice)); // written only when every codeblock CRC passes
  }
  if (uci_bytes != 0) {
    HIP_TRY(hipMemcpy(dv[2] + uci_off, uci_bits, uci_bytes, hipMemcpyHostToDevice));
  }
  if (csi2_bytes != 0) {
    HIP_TRY(hipMemcpy(dv[2] + csi2_off, csi2_bits, csi2_bytes, hipMemcpyHostToDevice)); // bytes behind the selected size stay
  }
  const uint32_t           zero = 0;
  const uint64_t           soft_o = 0, state_o = soft_room, tb_o = 0, uci_o = uci_off, csi2_o = csi2_off;
  nrphy_pusch_csi2_plan_t* plan = nullptr;
  rc = nrphy_pusch_csi2_plan_create(ctx, 1, pdu, desc, options, &zero, 1, grid_nof_ports, grid_nof_subc, &soft_o, &state_o, &tb_o, &uci_o,
                                    &csi2_o, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  auto* d_result = (nrphy_pusch_result_t*)dv[3];
  auto* d_csi2   = (nrphy_pusch_csi2_result_t*)(dv[3] + align_up(sizeof(nrphy_pusch_result_t)));
  rc = nrphy_pusch_csi2_run(plan, dv[0], dv[1], dv[2], dv[2], d_result, d_csi2, ctx->stream);
  if (rc == NRPHY_OK &&
      (call.sync() != hipSuccess || hipMemcpy(result, d_result, sizeof(*result), hipMemcpyDeviceToHost) != hipSuccess ||
       hipMemcpy(csi2_result, d_csi2, sizeof(*csi2_result), hipMemcpyDeviceToHost) != hipSuccess ||
       (has_decoder && (hipMemcpy(harq_soft, dv[1], soft_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(harq_state, dv[1] + soft_room, state_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(tb, dv[2], pdu->tb_size_bytes, hipMemcpyDeviceToHost) != hipSuccess)) ||
       (uci_bytes != 0 && hipMemcpy(uci_bits, dv[2] + uci_off, uci_bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
       (csi2_bytes != 0 && hipMemcpy(csi2_bits, dv[2] + csi2_off, csi2_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pusch_csi2_plan_destroy(plan);
  if (rc == NRPHY_OK) {
    result->harq_ack_offset -= (result->nof_harq_ack != 0 ? uci_off : 0); // relative to uci_bits
    result->csi_part1_offset -= (result->nof_csi_part1 != 0 ? uci_off : 0);
    csi2_result->csi_part2_offset = 0;                                   // relative to csi2_bits
  }
  return rc;
}
