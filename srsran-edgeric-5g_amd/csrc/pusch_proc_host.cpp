// Host side of the PUSCH processor (pusch_proc_kernels.hip): what pusch_processor_impl::process does before and between its
// stages (R/lib/phy/upper/channel_processors/pusch/pusch_processor_impl.cpp:115-336) -- the checks of assert_pdu and of the PDU
// validator, the UL-SCH information, one PDU turned into the configurations of the estimator, the demodulator, the demultiplexer,
// the UCI decoders and the transport-block decoder -- and the plan that owns the stage plans and the buffers between them.  The
// stages themselves are the library's: this file launches nothing but the result kernel.  One implementation serves
// nrphy_pusch_proc_*, nrphy_pusch_evm_* and nrphy_pusch_tp_*: the first are the second with enable_evm = 0, the second the third
// without a transform-precoding descriptor.
#include "ldpc_receive_host.h"
#include "pusch_alloc_host.h"
#include "pusch_proc_plan_host.h"
#include "ulsch_info_host.h"

#include <cmath>

namespace {

constexpr uint64_t ALIGN = 256;

uint64_t align_up(uint64_t v, uint64_t a = ALIGN)
{
  return (v + a - 1) / a * a;
}

// The options of a nrphy_pusch_proc_* call as those of its nrphy_pusch_evm_* namesake (null stays null).
struct WithoutEvm {
  nrphy_pusch_evm_options_t        value;
  const nrphy_pusch_evm_options_t* ptr;
  explicit WithoutEvm(const nrphy_pusch_proc_options_t* o) : value{}, ptr(o != nullptr ? &value : nullptr)
  {
    if (o != nullptr) {
      value.proc = *o;
    }
  }
};

bool transform_precoded(const nrphy_pusch_tp_desc_t* tp)
{
  return tp != nullptr && tp->transform_precoding != 0;
}

// The feature mask of the demodulator's _ex forms for a PDU (a plan: for any of its PDUs) with transform precoding.
constexpr uint32_t TP_DEMOD_FEATURES = NRPHY_PUSCH_DEMOD_TRANSFORM_PRECODING | NRPHY_PUSCH_DEMOD_PI2_BPSK;

// tp (may be null): the PDU's transform-precoding descriptor; lp: the estimator's low-PAPR DM-RS description that goes with d.chest.
int derive(const nrphy_pusch_pdu_t* p, const nrphy_pusch_tp_desc_t* tp, const nrphy_pusch_evm_options_t* eo, uint32_t grid_nof_ports,
           uint32_t grid_nof_subc, nrphy_pusch_proc_derived_t& d, nrphy_pusch_chest_lowpapr_t& lp)
{
  std::memset(&d, 0, sizeof(d));
  lp = {0, 0};
  if (p == nullptr || eo == nullptr || (tp != nullptr && tp->transform_precoding > 1)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const bool tpre = transform_precoded(tp);
  if (tpre) {
    lp = {1, tp->n_rs_id};
  }
  const nrphy_pusch_proc_options_t* o = &eo->proc;
  // The processor's configuration; the EVM-based SINR needs the EVM.
  if (o->dec_nof_iterations == 0 || o->dec_enable_early_stop > 1 || eo->enable_evm > 1 || eo->reserved_ != 0 ||
      (o->csi_sinr_calc_method != NRPHY_PUSCH_SINR_CHANNEL_ESTIMATOR && o->csi_sinr_calc_method != NRPHY_PUSCH_SINR_POST_EQUALIZATION &&
       !(o->csi_sinr_calc_method == NRPHY_PUSCH_SINR_EVM && eo->enable_evm == 1)) ||
      (o->equalizer != NRPHY_EQ_ZF && o->equalizer != NRPHY_EQ_MMSE)) {
    return NRPHY_ERR_ARGUMENT;
  }
  // assert_pdu and the PDU validator; what is out of scope.
  if (p->dmrs_type != 1 || p->nof_cdm_groups_without_data != 2 || p->nof_tx_layers < 1 ||
      p->nof_tx_layers > NRPHY_PUSCH_CHEST_MAX_LAYERS || p->tbs_lbrm_bytes == 0 || p->nof_csi_part2_entries != 0 ||
      p->has_codeword > 1 || (p->has_codeword != 0) != (p->tb_size_bytes != 0) || p->new_data > 1 ||
      (p->has_codeword == 0 && p->nof_harq_ack == 0 && p->nof_csi_part1 == 0) ||
      (p->modulation != NRPHY_MOD_QPSK && p->modulation != NRPHY_MOD_QAM16 && p->modulation != NRPHY_MOD_QAM64 &&
       p->modulation != NRPHY_MOD_QAM256 && !(tpre && p->modulation == NRPHY_MOD_PI2_BPSK)) ||
      (p->has_codeword != 0 && (p->rv > 3 || (p->ldpc_base_graph != 1 && p->ldpc_base_graph != 2)))) {
    return NRPHY_ERR_ARGUMENT;
  }
  const uint32_t qm = p->modulation == NRPHY_MOD_PI2_BPSK ? 1 : p->modulation;

  nrphy_pusch_chest_cfg_t& ce = d.chest;
  ce.numerology         = p->numerology;
  ce.slot_index         = p->slot_index;
  ce.scrambling_id      = p->scrambling_id;
  ce.n_scid             = p->n_scid;
  ce.scaling            = (float)std::pow(10.0, 3.0 / 20.0); // convert_dB_to_amplitude(-get_sch_to_dmrs_ratio_dB(2)), ratio -3 dB
  ce.dmrs_type          = p->dmrs_type;
  ce.dmrs_symbol_mask   = p->dmrs_symbol_mask;
  ce.start_symbol_index = p->start_symbol_index;
  ce.nof_symbols        = p->nof_symbols;
  ce.nof_tx_layers      = p->nof_tx_layers;
  ce.nof_rx_ports       = p->nof_rx_ports;
  ce.dc_position        = p->dc_position;
  std::memcpy(ce.rx_ports, p->rx_ports, sizeof(ce.rx_ports));
  std::memcpy(ce.prb_mask, p->prb_mask, sizeof(ce.prb_mask));

  nrphy_pusch_demod_cfg_t& dm = d.demod;
  dm.rnti                        = p->rnti;
  dm.n_id                        = p->n_id;
  dm.qm                          = qm;
  dm.start_symbol_index          = p->start_symbol_index;
  dm.nof_symbols                 = p->nof_symbols;
  dm.dmrs_symbol_mask            = p->dmrs_symbol_mask;
  dm.dmrs_type                   = p->dmrs_type;
  dm.nof_cdm_groups_without_data = p->nof_cdm_groups_without_data;
  dm.nof_tx_layers               = p->nof_tx_layers;
  dm.nof_rx_ports                = p->nof_rx_ports;
  dm.equalizer                   = o->equalizer;
  dm.transform_precoding         = tpre ? 1 : 0; // 0: pusch_processor_impl.cpp:294
  std::memcpy(dm.rx_ports, p->rx_ports, sizeof(dm.rx_ports));
  std::memcpy(dm.prb_mask, p->prb_mask, sizeof(dm.prb_mask));
  if (nrphy_pusch_chest_validate_ex(&ce, &lp, grid_nof_ports, grid_nof_subc) != NRPHY_OK ||
      nrphy_pusch_demod_validate_ex(&dm, grid_nof_ports, grid_nof_subc, tpre ? TP_DEMOD_FEATURES : 0) != NRPHY_OK ||
      p->rnti > 65535U || p->n_id > 1023U) {
    return NRPHY_ERR_ARGUMENT;
  }
  d.codeword_bits = (uint32_t)nrphy_pusch_demod_codeword_bits(&dm);

  // get_ulsch_information as if there were no CSI part 2 (pusch_processor_impl.cpp:138-164).
  const uint32_t nof_rb = nof_prb(pusch_allocation(ce));
  const nrphy_ulsch_info_cfg_t ic = pusch_proc_info_cfg(*p, nof_rb, 0);
  if (p->tb_size_bytes > NRPHY_MAX_TB_BYTES || ulsch_info(ic, d.info) != NRPHY_OK) {
    return NRPHY_ERR_ARGUMENT;
  }

  // The demultiplexer (pusch_processor_impl.cpp:204-218) and the UCI decoders.
  nrphy_ulsch_demux_cfg_t& dx = d.demux;
  dx.modulation                  = p->modulation;
  dx.nof_layers                  = p->nof_tx_layers;
  dx.nof_prb                     = nof_rb;
  dx.start_symbol_index          = p->start_symbol_index;
  dx.nof_symbols                 = p->nof_symbols;
  dx.dmrs_type                   = p->dmrs_type - 1; // the demultiplexer's code: 0 = type 1
  dx.dmrs_symbol_mask            = p->dmrs_symbol_mask;
  dx.nof_cdm_groups_without_data = p->nof_cdm_groups_without_data;
  dx.nof_harq_ack_rvd            = d.info.nof_harq_ack_rvd;
  dx.nof_harq_ack_bits           = p->nof_harq_ack;
  dx.nof_enc_harq_ack_bits       = d.info.nof_harq_ack_bits;
  dx.nof_csi_part1_bits          = p->nof_csi_part1;
  dx.nof_enc_csi_part1_bits      = d.info.nof_csi_part1_bits;
  dx.rnti                        = p->rnti;
  dx.n_id                        = p->n_id;
  if (p->nof_harq_ack != 0) {
    d.uci[d.nof_uci++] = {p->nof_harq_ack, d.info.nof_harq_ack_bits, p->modulation, 0};
  }
  if (p->nof_csi_part1 != 0) {
    d.uci[d.nof_uci++] = {p->nof_csi_part1, d.info.nof_csi_part1_bits, p->modulation, 0};
  }
  d.nof_sch_bits = d.codeword_bits;
  if (d.nof_uci != 0) {
    nrphy_ulsch_demux_sizes_t sizes;
    if (nrphy_ulsch_demux_sizes(&dx, &sizes) != NRPHY_OK || sizes.nof_codeword_bits != d.codeword_bits) {
      return NRPHY_ERR_ARGUMENT;
    }
    d.nof_sch_bits = sizes.nof_sch_bits;
    for (uint32_t k = 0; k != d.nof_uci; ++k) {
      if (nrphy_uci_decoder_validate(&d.uci[k]) != NRPHY_OK) {
        return NRPHY_ERR_ARGUMENT;
      }
    }
  }

  // The transport-block decoder (pusch_processor_impl.cpp:239-264).
  if (p->has_codeword != 0) {
    if (d.info.nof_ul_sch_bits != d.nof_sch_bits || d.nof_sch_bits == 0) {
      return NRPHY_ERR_ARGUMENT;
    }
    const uint32_t b      = 8 * p->tb_size_bytes + (8 * p->tb_size_bytes <= 3824 ? 16 : 24);
    const uint32_t kcb    = p->ldpc_base_graph == 1 ? 8448 : 3840;
    const uint32_t nof_cb = b <= kcb ? 1 : divide_ceil(b, kcb - 24); // ldpc::compute_nof_codeblocks
    nrphy_pusch_decoder_cfg_t& dc = d.decoder;
    dc.base_graph     = p->ldpc_base_graph;
    dc.qm             = qm;
    dc.rv             = p->rv;
    dc.nof_layers     = p->nof_tx_layers;
    dc.nref           = (uint32_t)std::min<uint64_t>((uint64_t)p->tbs_lbrm_bytes * 8 * 3 / (2 * nof_cb), 66 * 384); // ldpc::compute_N_ref
    dc.tb_size_bytes  = p->tb_size_bytes;
    dc.nof_ch_symbols = d.nof_sch_bits / qm;
    dc.max_iterations = o->dec_nof_iterations;
    dc.use_early_stop = o->dec_enable_early_stop;
    dc.new_data       = p->new_data;
    uint64_t soft = 0, state = 0;
    uint32_t ncb = 0;
    if (dc.nref == 0 || !pusch_decoder_harq_sizes(dc, 1, &soft, &state, &ncb)) {
      return NRPHY_ERR_ARGUMENT;
    }
    d.has_decoder = 1;
  }
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_ul_sch_info(const nrphy_ulsch_info_cfg_t* cfg, nrphy_ulsch_info_t* out)
{
  if (cfg == nullptr || out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  return ulsch_info(*cfg, *out);
}

extern "C" int nrphy_pusch_proc_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options,
                                         uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return nrphy_pusch_tp_validate(pdu, nullptr, WithoutEvm(options).ptr, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_pusch_evm_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_evm_options_t* options,
                                        uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  return nrphy_pusch_tp_validate(pdu, nullptr, options, grid_nof_ports, grid_nof_subc);
}

extern "C" int nrphy_pusch_tp_validate(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp,
                                       const nrphy_pusch_evm_options_t* options, uint32_t grid_nof_ports, uint32_t grid_nof_subc)
{
  nrphy_pusch_proc_derived_t  d;
  nrphy_pusch_chest_lowpapr_t lp;
  return derive(pdu, tp, options, grid_nof_ports, grid_nof_subc, d, lp);
}

extern "C" int nrphy_pusch_proc_derive(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options,
                                       uint32_t grid_nof_ports, uint32_t grid_nof_subc, nrphy_pusch_proc_derived_t* out)
{
  return nrphy_pusch_tp_derive(pdu, nullptr, WithoutEvm(options).ptr, grid_nof_ports, grid_nof_subc, out, nullptr);
}

extern "C" int nrphy_pusch_tp_derive(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp,
                                     const nrphy_pusch_evm_options_t* options, uint32_t grid_nof_ports, uint32_t grid_nof_subc,
                                     nrphy_pusch_proc_derived_t* out, nrphy_pusch_chest_lowpapr_t* lp_out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  nrphy_pusch_chest_lowpapr_t lp;
  const int                   rc = derive(pdu, tp, options, grid_nof_ports, grid_nof_subc, *out, lp);
  if (rc != NRPHY_OK) {
    std::memset(out, 0, sizeof(*out));
    lp = {0, 0};
  }
  if (lp_out != nullptr) {
    *lp_out = lp;
  }
  return rc;
}

extern "C" int nrphy_pusch_proc_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options,
                                           uint64_t* soft_bytes, uint64_t* state_bytes)
{
  return nrphy_pusch_tp_harq_bytes(pdu, nullptr, WithoutEvm(options).ptr, soft_bytes, state_bytes);
}

extern "C" int nrphy_pusch_tp_harq_bytes(const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp,
                                         const nrphy_pusch_evm_options_t* options, uint64_t* soft_bytes, uint64_t* state_bytes)
{
  if (pdu == nullptr || soft_bytes == nullptr || state_bytes == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  // The sizes do not depend on the grid: the smallest one that holds the PDU's allocation and ports.
  uint32_t ports = 1;
  for (uint32_t i = 0; i != std::min<uint32_t>(pdu->nof_rx_ports, NRPHY_MAX_PORTS); ++i) {
    ports = std::max(ports, std::min<uint32_t>(pdu->rx_ports[i], NRPHY_MAX_PORTS - 1) + 1);
  }
  uint32_t subc = (uint32_t)(mask_highest(pdu->prb_mask) + 1) * NRPHY_NRE;
  if (pdu->dc_position != NRPHY_PUSCH_CHEST_NO_DC) {
    subc = std::max(subc, std::min<uint32_t>(pdu->dc_position / NRPHY_NRE + 1, NRPHY_MAX_RB) * NRPHY_NRE);
  }
  nrphy_pusch_proc_derived_t  d;
  nrphy_pusch_chest_lowpapr_t lp;
  const int                   rc = derive(pdu, tp, options, ports, subc, d, lp);
  if (rc != NRPHY_OK) {
    return rc;
  }
  *soft_bytes = *state_bytes = 0;
  uint32_t ncb = 0;
  if (d.has_decoder != 0 && !pusch_decoder_harq_sizes(d.decoder, 1, soft_bytes, state_bytes, &ncb)) {
    return NRPHY_ERR_ARGUMENT;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_proc_plan_destroy(nrphy_pusch_proc_plan_t* plan)
{
  if (plan == nullptr) {
    return NRPHY_OK;
  }
  nrphy_pusch_chest_plan_destroy(plan->chest);
  nrphy_pusch_demod_plan_destroy(plan->demod);
  nrphy_ulsch_demux_plan_destroy(plan->demux);
  nrphy_uci_decoder_plan_destroy(plan->uci);
  if (plan->d_arena != nullptr) {
    (void)hipSetDevice(plan->ctx->device);
    (void)hipFree(plan->d_arena);
  }
  delete plan;
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_proc_plan_harq_bytes(const nrphy_pusch_proc_plan_t* plan, uint32_t i, uint64_t* soft_bytes,
                                                uint64_t* state_bytes)
{
  if (plan == nullptr || i >= plan->n || soft_bytes == nullptr || state_bytes == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *soft_bytes  = plan->soft_bytes[i];
  *state_bytes = plan->state_bytes[i];
  return NRPHY_OK;
}

namespace {
// The plan of PDUs whose records are at hand: `pre` (may be null) holds one accepted derivation per PDU, so that a caller that
// derived already -- the host form -- does not derive again.
int plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_tp_desc_t* tps,
                const nrphy_pusch_evm_options_t* options, const nrphy_pusch_proc_derived_t* pre, const uint32_t* grid_index, uint32_t nof_grids, uint32_t grid_nof_ports,
                uint32_t grid_nof_subc, const uint64_t* harq_soft_offset, const uint64_t* harq_state_offset, const uint64_t* tb_offset,
                const uint64_t* uci_offset, nrphy_pusch_proc_plan_t** out)
{
  if (out == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  *out = nullptr;
  if (ctx == nullptr || n == 0 || n > 65535U || pdus == nullptr || options == nullptr || grid_index == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  std::vector<nrphy_pusch_proc_derived_t> derived(n);
  std::vector<nrphy_pusch_chest_cfg_t>    chest(n);
  std::vector<nrphy_pusch_chest_lowpapr_t> lowpapr(n, nrphy_pusch_chest_lowpapr_t{0, 0});
  bool                                    any_tp = false;
  std::vector<nrphy_pusch_demod_cfg_t>    demod(n);
  std::vector<uint64_t>                   ce_offset(n);
  std::vector<PuschProcDesc>              desc(n);
  std::vector<nrphy_ulsch_demux_cfg_t>    demux;
  std::vector<uint64_t>                   dx_in, dx_sch, dx_harq, dx_csi1;
  std::vector<nrphy_uci_decoder_cfg_t>    uci;
  std::vector<uint64_t>                   uci_llr, uci_msg;
  auto*                                   plan = new nrphy_pusch_proc_plan;
  plan->ctx = ctx;
  plan->n   = n;
  plan->soft_bytes.assign(n, 0);
  plan->state_bytes.assign(n, 0);
  uint64_t ce_words = 0, sch_bytes = 0, uci_llr_bytes = 0, scratch_bytes = 0;
  int      rc = NRPHY_OK;
  for (uint32_t i = 0; i != n && rc == NRPHY_OK; ++i) {
    nrphy_pusch_proc_derived_t& d = derived[i];
    const nrphy_pusch_tp_desc_t* tp = tps != nullptr ? &tps[i] : nullptr;
    if (pre != nullptr) {
      d = pre[i];
      if (transform_precoded(tp)) {
        lowpapr[i] = {1, tp->n_rs_id};
      }
    } else if ((rc = derive(&pdus[i], tp, options, grid_nof_ports, grid_nof_subc, d, lowpapr[i])) != NRPHY_OK) {
      break;
    }
    any_tp = any_tp || transform_precoded(tp);
    if (grid_index[i] >= nof_grids || (d.nof_uci != 0 && uci_offset == nullptr) ||
        (d.has_decoder != 0 && (harq_soft_offset == nullptr || harq_state_offset == nullptr || tb_offset == nullptr ||
                                harq_state_offset[i] % 64 != 0))) {
      rc = NRPHY_ERR_ARGUMENT;
      break;
    }
    chest[i]     = d.chest;
    demod[i]     = d.demod;
    ce_offset[i] = ce_words;
    ce_words += (uint64_t)d.chest.nof_tx_layers * d.chest.nof_rx_ports * NRPHY_NSYMB * grid_nof_subc;
    plan->llr_stride = std::max<uint64_t>(plan->llr_stride, align_up(d.codeword_bits, 16));
    PuschProcDesc& pd = desc[i];
    std::memset(&pd, 0, sizeof(pd));
    pd.nof_rx_ports = d.chest.nof_rx_ports;
    pd.has_sch      = d.has_decoder;
    pd.harq_status = pd.csi1_status = PUSCH_PROC_NO_STATUS;
    pd.sinr_method                  = options->proc.csi_sinr_calc_method;
    pd.has_evm                      = options->enable_evm;
  }
  // Offsets that need the common codeword stride.
  for (uint32_t i = 0; i != n && rc == NRPHY_OK; ++i) {
    const nrphy_pusch_proc_derived_t& d  = derived[i];
    PuschProcDesc&                    pd = desc[i];
    uint64_t                          sch_at = 0;
    if (d.nof_uci != 0) {
      sch_at = sch_bytes;
      sch_bytes += align_up(d.nof_sch_bits, 16);
      demux.push_back(d.demux);
      dx_in.push_back(i * plan->llr_stride);
      dx_sch.push_back(sch_at);
      dx_harq.push_back(0);
      dx_csi1.push_back(0);
      uint64_t msg_at = uci_offset[i];
      for (uint32_t k = 0; k != d.nof_uci; ++k) {
        const bool is_harq = (k == 0 && pdus[i].nof_harq_ack != 0);
        (is_harq ? dx_harq : dx_csi1).back() = uci_llr_bytes;
        (is_harq ? pd.harq_status : pd.csi1_status) = (uint32_t)uci.size();
        (is_harq ? pd.harq_ack_offset : pd.csi_part1_offset) = msg_at;
        (is_harq ? pd.nof_harq_ack : pd.nof_csi_part1) = d.uci[k].message_length;
        uci.push_back(d.uci[k]);
        uci_llr.push_back(uci_llr_bytes);
        uci_msg.push_back(msg_at);
        uci_llr_bytes += align_up(d.uci[k].llr_length, 16);
        msg_at += d.uci[k].message_length;
      }
    }
    if (d.has_decoder != 0) {
      ProcDecoder dec;
      dec.cfg          = d.decoder;
      dec.pdu          = i;
      dec.from_sch     = d.nof_uci != 0;
      dec.llr_offset   = dec.from_sch ? sch_at : i * plan->llr_stride;
      dec.soft_offset  = harq_soft_offset[i];
      dec.state_offset = harq_state_offset[i];
      dec.tb_offset    = tb_offset[i];
      uint64_t scratch = 0;
      if (nrphy_pusch_decoder_sizes(ctx, &dec.cfg, 1, &plan->soft_bytes[i], &plan->state_bytes[i], &scratch, &pd.nof_codeblocks) !=
          NRPHY_OK) {
        rc = NRPHY_ERR_ARGUMENT;
        break;
      }
      scratch_bytes = std::max(scratch_bytes, scratch);
      plan->decoders.push_back(dec);
    }
  }
  if (rc == NRPHY_OK) {
    rc = nrphy_pusch_chest_plan_create_ex(ctx, n, chest.data(), any_tp ? lowpapr.data() : nullptr, grid_index, nof_grids, grid_nof_ports,
                                          grid_nof_subc, ce_offset.data(), &plan->chest);
  }
  if (rc == NRPHY_OK) {
    rc = nrphy_pusch_demod_plan_create_ex(ctx, n, demod.data(), grid_index, nof_grids, grid_nof_ports, grid_nof_subc, ce_offset.data(),
                                          any_tp ? TP_DEMOD_FEATURES : 0, &plan->demod);
  }
  if (rc == NRPHY_OK && !demux.empty()) {
    rc = nrphy_ulsch_demux_plan_create(ctx, (uint32_t)demux.size(), demux.data(), dx_in.data(), dx_sch.data(), dx_harq.data(),
                                       dx_csi1.data(), nullptr, &plan->demux);
  }
  if (rc == NRPHY_OK && !uci.empty()) {
    rc = nrphy_uci_decoder_plan_create(ctx, (uint32_t)uci.size(), uci.data(), uci_llr.data(), uci_msg.data(), &plan->uci);
  }
  for (size_t k = 0; k != plan->decoders.size() && rc == NRPHY_OK; ++k) {
    rc = nrphy_pusch_decoder_prepare(ctx, &plan->decoders[k].cfg);
  }
  if (rc != NRPHY_OK) {
    nrphy_pusch_proc_plan_destroy(plan);
    return rc;
  }
  // One allocation: the descriptors, then the workspace.
  const uint64_t piece[] = {ce_words * 4,
                            (uint64_t)n * NRPHY_MAX_PORTS * sizeof(float),
                            (uint64_t)n * NRPHY_MAX_PORTS * NRPHY_PUSCH_CHEST_MAX_LAYERS * sizeof(nrphy_pusch_chest_meas_t),
                            (uint64_t)n * sizeof(float),
                            (uint64_t)n * plan->llr_stride,
                            sch_bytes,
                            uci_llr_bytes,
                            (uint64_t)n * 4 * sizeof(uint32_t),
                            (uint64_t)uci.size() * sizeof(uint32_t),
                            scratch_bytes,
                            (uint64_t)n * sizeof(float)};
  constexpr size_t NP = sizeof(piece) / sizeof(piece[0]);
  uint64_t         at[NP + 1] = {};
  for (size_t k = 0; k != NP; ++k) {
    at[k + 1] = at[k] + align_up(std::max<uint64_t>(piece[k], 16));
  }
  plan->desc = desc;
  DeviceArena arena;
  arena.add(&plan->d_desc, desc.data(), desc.size() * sizeof(PuschProcDesc));
  uint8_t* ws = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || arena.commit(&plan->d_arena, at[NP], (void**)&ws) != hipSuccess ||
      hipMemset(ws, 0, at[NP]) != hipSuccess) { // ports a PDU does not have and PDUs without codeword read as zeros
    nrphy_pusch_proc_plan_destroy(plan);
    return NRPHY_ERR_DEVICE;
  }
  plan->d_ce      = (uint32_t*)(ws + at[0]);
  plan->d_nv      = (float*)(ws + at[1]);
  plan->d_meas    = (nrphy_pusch_chest_meas_t*)(ws + at[2]);
  plan->d_sinr    = (float*)(ws + at[3]);
  plan->d_llr     = (int8_t*)(ws + at[4]);
  plan->d_sch     = (int8_t*)(ws + at[5]);
  plan->d_uci_llr = (int8_t*)(ws + at[6]);
  plan->d_dec     = (uint32_t*)(ws + at[7]);
  plan->d_status  = (uint32_t*)(ws + at[8]);
  plan->d_scratch = ws + at[9];
  plan->d_evm     = options->enable_evm != 0 ? (float*)(ws + at[10]) : nullptr;
  *out            = plan;
  return NRPHY_OK;
}

} // namespace

extern "C" int nrphy_pusch_proc_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                            const nrphy_pusch_proc_options_t* options, const uint32_t* grid_index, uint32_t nof_grids,
                                            uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* harq_soft_offset,
                                            const uint64_t* harq_state_offset, const uint64_t* tb_offset, const uint64_t* uci_offset,
                                            nrphy_pusch_proc_plan_t** out)
{
  return plan_create(ctx, n, pdus, nullptr, WithoutEvm(options).ptr, nullptr, grid_index, nof_grids, grid_nof_ports, grid_nof_subc,
                     harq_soft_offset, harq_state_offset, tb_offset, uci_offset, out);
}

extern "C" int nrphy_pusch_evm_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus,
                                           const nrphy_pusch_evm_options_t* options, const uint32_t* grid_index, uint32_t nof_grids,
                                           uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* harq_soft_offset,
                                           const uint64_t* harq_state_offset, const uint64_t* tb_offset, const uint64_t* uci_offset,
                                           nrphy_pusch_proc_plan_t** out)
{
  return plan_create(ctx, n, pdus, nullptr, options, nullptr, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, harq_soft_offset,
                     harq_state_offset, tb_offset, uci_offset, out);
}

extern "C" int nrphy_pusch_tp_plan_create(nrphy_ctx_t* ctx, uint32_t n, const nrphy_pusch_pdu_t* pdus, const nrphy_pusch_tp_desc_t* tps,
                                          const nrphy_pusch_evm_options_t* options, const uint32_t* grid_index, uint32_t nof_grids,
                                          uint32_t grid_nof_ports, uint32_t grid_nof_subc, const uint64_t* harq_soft_offset,
                                          const uint64_t* harq_state_offset, const uint64_t* tb_offset, const uint64_t* uci_offset,
                                          nrphy_pusch_proc_plan_t** out)
{
  return plan_create(ctx, n, pdus, tps, options, nullptr, grid_index, nof_grids, grid_nof_ports, grid_nof_subc, harq_soft_offset,
                     harq_state_offset, tb_offset, uci_offset, out);
}

int pusch_proc_run_front(nrphy_pusch_proc_plan_t* plan, const void* d_grid, uint8_t* d_uci_bits, void* stream)
{
  int rc = nrphy_pusch_chest_run(plan->chest, d_grid, plan->d_ce, plan->d_nv, plan->d_meas, stream);
  if (rc == NRPHY_OK) {
    rc = nrphy_pusch_demod_run_evm(plan->demod, d_grid, plan->d_ce, plan->d_nv, plan->d_llr, plan->llr_stride, plan->d_sinr,
                                   plan->d_evm, stream); // d_evm null: nrphy_pusch_demod_run
  }
  if (rc == NRPHY_OK && plan->demux != nullptr) {
    rc = nrphy_ulsch_demux_run(plan->demux, plan->d_llr, plan->d_sch, plan->d_uci_llr, plan->d_uci_llr, nullptr, stream);
  }
  if (rc == NRPHY_OK && plan->uci != nullptr) {
    rc = nrphy_uci_decoder_run(plan->uci, plan->d_uci_llr, d_uci_bits, plan->d_status, stream);
  }
  return rc;
}

int pusch_proc_run_decoder(nrphy_pusch_proc_plan_t* plan, size_t k, void* d_harq, uint8_t* d_tb, void* stream)
{
  const ProcDecoder& dec = plan->decoders[k];
  return nrphy_pusch_decode_batch(plan->ctx, &dec.cfg, 1, (dec.from_sch ? plan->d_sch : plan->d_llr) + dec.llr_offset,
                                  (uint64_t)dec.cfg.nof_ch_symbols * dec.cfg.qm, (int8_t*)d_harq + dec.soft_offset,
                                  (uint8_t*)d_harq + dec.state_offset, plan->d_scratch, d_tb + dec.tb_offset, dec.cfg.tb_size_bytes,
                                  plan->d_dec + 4 * (size_t)dec.pdu, stream);
}

int pusch_proc_run_result(nrphy_pusch_proc_plan_t* plan, nrphy_pusch_result_t* d_result, void* stream)
{
  PuschProcLaunch p;
  p.desc    = plan->d_desc;
  p.meas    = plan->d_meas;
  p.sinr_db = plan->d_sinr;
  p.dec     = plan->d_dec;
  p.status  = plan->d_status;
  p.result  = d_result;
  p.n       = plan->n;
  p.evm     = plan->d_evm;
  HIP_TRY(hipSetDevice(plan->ctx->device));
  HIP_TRY(launch_pusch_proc_result(p, stream ? (hipStream_t)stream : plan->ctx->stream));
  return NRPHY_OK;
}

bool pusch_proc_run_arguments_ok(const nrphy_pusch_proc_plan_t* plan, const void* d_grid, const void* d_harq, const uint8_t* d_tb,
                                 const uint8_t* d_uci_bits, const nrphy_pusch_result_t* d_result)
{
  return !(plan == nullptr || d_grid == nullptr || d_result == nullptr || ((uintptr_t)d_result & 7U) != 0 ||
           (!plan->decoders.empty() && (d_harq == nullptr || d_tb == nullptr || ((uintptr_t)d_harq & 63U) != 0)) ||
           (plan->uci != nullptr && d_uci_bits == nullptr));
}

extern "C" int nrphy_pusch_proc_run(nrphy_pusch_proc_plan_t* plan, const void* d_grid, void* d_harq, uint8_t* d_tb, uint8_t* d_uci_bits,
                                    nrphy_pusch_result_t* d_result, void* stream)
{
  if (!pusch_proc_run_arguments_ok(plan, d_grid, d_harq, d_tb, d_uci_bits, d_result)) {
    return NRPHY_ERR_ARGUMENT;
  }
  int rc = pusch_proc_run_front(plan, d_grid, d_uci_bits, stream);
  for (size_t k = 0; k != plan->decoders.size() && rc == NRPHY_OK; ++k) {
    rc = pusch_proc_run_decoder(plan, k, d_harq, d_tb, stream);
  }
  return rc != NRPHY_OK ? rc : pusch_proc_run_result(plan, d_result, stream);
}

extern "C" int nrphy_pusch_proc_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_proc_options_t* options,
                                     const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, int8_t* harq_soft,
                                     uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits, nrphy_pusch_result_t* result)
{
  return nrphy_pusch_evm_host(ctx, pdu, WithoutEvm(options).ptr, grid, grid_nof_ports, grid_nof_subc, harq_soft, harq_state, tb,
                              uci_bits, result);
}

extern "C" int nrphy_pusch_evm_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_evm_options_t* options,
                                    const void* grid, uint32_t grid_nof_ports, uint32_t grid_nof_subc, int8_t* harq_soft,
                                    uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits, nrphy_pusch_result_t* result)
{
  return nrphy_pusch_tp_host(ctx, pdu, nullptr, options, grid, grid_nof_ports, grid_nof_subc, harq_soft, harq_state, tb, uci_bits,
                             result);
}

extern "C" int nrphy_pusch_tp_host(nrphy_ctx_t* ctx, const nrphy_pusch_pdu_t* pdu, const nrphy_pusch_tp_desc_t* tp,
                                   const nrphy_pusch_evm_options_t* options, const void* grid, uint32_t grid_nof_ports,
                                   uint32_t grid_nof_subc, int8_t* harq_soft, uint8_t* harq_state, uint8_t* tb, uint8_t* uci_bits,
                                   nrphy_pusch_result_t* result)
{
  nrphy_pusch_proc_derived_t  d;
  nrphy_pusch_chest_lowpapr_t lp;
  if (ctx == nullptr || grid == nullptr || result == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  int rc = derive(pdu, tp, options, grid_nof_ports, grid_nof_subc, d, lp);
  if (rc != NRPHY_OK) {
    return rc;
  }
  uint64_t soft_bytes = 0, state_bytes = 0;
  uint32_t ncb = 0;
  if (d.has_decoder != 0 && (harq_soft == nullptr || harq_state == nullptr || tb == nullptr ||
                             !pusch_decoder_harq_sizes(d.decoder, 1, &soft_bytes, &state_bytes, &ncb))) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t uci_bytes = pdu->nof_harq_ack + pdu->nof_csi_part1;
  if (uci_bytes != 0 && uci_bits == nullptr) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t grid_bytes = (size_t)grid_nof_ports * NRPHY_NSYMB * grid_nof_subc * 4;
  const size_t soft_room  = align_up(soft_bytes);
  HostCall call(ctx);
  uint8_t* dv[4]; // grid, HARQ arena (soft block, then state block), transport block + UCI payload, result
  if (!call.carve(SCRATCH_RX, {grid_bytes, soft_room + (size_t)state_bytes, align_up(pdu->tb_size_bytes) + uci_bytes,
                               sizeof(nrphy_pusch_result_t)}, dv)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(dv[0], grid, grid_bytes, hipMemcpyHostToDevice));
  if (d.has_decoder != 0) {
    HIP_TRY(hipMemcpy(dv[1], harq_soft, soft_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv[1] + soft_room, harq_state, state_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dv[2], tb, pdu->tb_size_bytes, hipMemcpyHostToDevice)); // written only when every codeblock CRC passes
  }
  if (uci_bytes != 0) {
    HIP_TRY(hipMemcpy(dv[2] + align_up(pdu->tb_size_bytes), uci_bits, uci_bytes, hipMemcpyHostToDevice)); // a failed first polar block leaves the second as it was
  }
  const uint32_t           zero = 0;
  const uint64_t           soft_off = 0, state_off = soft_room, tb_off = 0, uci_off = align_up(pdu->tb_size_bytes);
  nrphy_pusch_proc_plan_t* plan = nullptr;
  rc = plan_create(ctx, 1, pdu, tp, options, &d, &zero, 1, grid_nof_ports, grid_nof_subc, &soft_off, &state_off, &tb_off, &uci_off, &plan);
  if (rc != NRPHY_OK) {
    return rc;
  }
  rc = nrphy_pusch_proc_run(plan, dv[0], dv[1], dv[2], dv[2], (nrphy_pusch_result_t*)dv[3], ctx->stream);
  if (rc == NRPHY_OK && (call.sync() != hipSuccess || hipMemcpy(result, dv[3], sizeof(*result), hipMemcpyDeviceToHost) != hipSuccess ||
                         (d.has_decoder != 0 && (hipMemcpy(harq_soft, dv[1], soft_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                                                 hipMemcpy(harq_state, dv[1] + soft_room, state_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                                                 hipMemcpy(tb, dv[2], pdu->tb_size_bytes, hipMemcpyDeviceToHost) != hipSuccess)) ||
                         (uci_bytes != 0 && hipMemcpy(uci_bits, dv[2] + uci_off, uci_bytes, hipMemcpyDeviceToHost) != hipSuccess))) {
    rc = NRPHY_ERR_DEVICE;
  }
  nrphy_pusch_proc_plan_destroy(plan);
  if (rc == NRPHY_OK) {
    result->harq_ack_offset -= (result->nof_harq_ack != 0 ? uci_off : 0); // relative to uci_bits
    result->csi_part1_offset -= (result->nof_csi_part1 != 0 ? uci_off : 0);
  }
  return rc;
}
