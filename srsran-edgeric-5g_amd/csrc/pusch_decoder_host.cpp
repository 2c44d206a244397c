// Host side of pusch_decoder.hip: the PUSCH transport-block decoder -- rate dematcher, LDPC decoder and the assembly kernel.
#include "ldpc_receive_host.h"
#include "nrphy_trace.h"
#include "pdsch_plan.h"

#include <cmath>

namespace {

struct PuschLayout {
  nrphy_pdsch_derived_t d;
  uint32_t              msg_stride; // bytes per decoded message
  uint64_t              off_ok, off_skip, off_iter, off_msg, state_bytes;
};

bool pusch_layout(const nrphy_pusch_decoder_cfg_t& cfg, uint32_t n_tb, PuschLayout& l)
{
  if ((cfg.base_graph != 1 && cfg.base_graph != 2) || (cfg.qm != 1 && cfg.qm != 2 && cfg.qm != 4 && cfg.qm != 6 && cfg.qm != 8) ||
      cfg.rv > 3 || cfg.nof_layers == 0 || cfg.nof_layers > NRPHY_MAX_LAYERS || cfg.tb_size_bytes == 0 ||
      cfg.tb_size_bytes > NRPHY_MAX_TB_BYTES || cfg.nof_ch_symbols == 0 || cfg.nof_ch_symbols % cfg.nof_layers != 0 || cfg.max_iterations == 0) {
    return false;
  }
  // Segmentation is the transmitter's (ldpc_segmenter_rx_impl mirrors ldpc_segmenter_tx): reuse its derivation.
  nrphy_pdsch_pdu_t pdu;
  std::memset(&pdu, 0, sizeof(pdu));
  pdu.ldpc_base_graph = cfg.base_graph;
  pdu.tb_size_bytes   = cfg.tb_size_bytes;
  pdu.rv              = cfg.rv;
  pdu.nof_layers      = cfg.nof_layers;
  pdu.qm              = cfg.qm;
  const uint32_t nref = cfg.nref;
  derive(pdu, cfg.nof_ch_symbols / cfg.nof_layers, l.d, &nref);
  if (l.d.lifting_size == 0 || l.d.nof_codeblocks == 0 || l.d.nof_codeblocks > NRPHY_MAX_CODEBLOCKS ||
      l.d.rm_length_short == 0) {
    return false;
  }
  const uint64_t n_cb = (uint64_t)n_tb * l.d.nof_codeblocks;
  l.msg_stride        = ((l.d.segment_length + 7) / 8 + 8 + 15) & ~15U;
  l.off_ok            = 0;
  l.off_skip          = (n_cb + 63) & ~(uint64_t)63;
  l.off_iter          = 2 * l.off_skip;
  l.off_msg           = (l.off_iter + 4 * n_cb + 63) & ~(uint64_t)63;
  l.state_bytes       = l.off_msg + n_cb * l.msg_stride;
  return true;
}

// Weights of the assembly kernel's per-thread transport-block CRC pieces (pusch_decoder.hip): fixed by the block size.
const uint32_t* get_pusch_tb_crc_weights(nrphy_ctx* ctx, uint32_t tb_size_bytes)
{
  std::lock_guard<std::recursive_mutex> lock(ctx->host_mutex);
  auto                                  it = ctx->d_tb_crc_w.find(tb_size_bytes);
  if (it == ctx->d_tb_crc_w.end()) {
    const uint32_t        piece = divide_ceil(tb_size_bytes, PUSCH_ASSEMBLE_THREADS);
    std::vector<uint32_t> w(PUSCH_ASSEMBLE_THREADS);
    for (uint32_t t = 0; t != PUSCH_ASSEMBLE_THREADS; ++t) {
      const uint32_t end = std::min<uint32_t>(std::min<uint32_t>(t * piece, tb_size_bytes) + piece, tb_size_bytes);
      w[t]               = CRC24A_FIELD.xpow(8 * (int64_t)(tb_size_bytes - end));
    }
    uint32_t* d_w = nullptr;
    if (upload(&d_w, w.data(), w.size() * sizeof(uint32_t)) != hipSuccess) {
      return nullptr;
    }
    it = ctx->d_tb_crc_w.emplace(tb_size_bytes, d_w).first;
  }
  return it->second;
}

nrphy_ldpc_decoder_cfg_t pusch_ldpc_cfg(const nrphy_pusch_decoder_cfg_t& cfg, const nrphy_pdsch_derived_t& d)
{
  // Decoding of the codeblocks whose CRC has not passed yet (pusch_codeblock_decoder.cpp:36-71): CRC24B per codeblock,
  // the transport block's own CRC when it is a single codeblock.
  nrphy_ldpc_decoder_cfg_t dec;
  dec.base_graph      = cfg.base_graph;
  dec.lifting_size    = d.lifting_size;
  dec.nof_filler_bits = d.nof_filler_bits;
  dec.crc_poly        = (d.nof_codeblocks > 1) ? 0x24B : (d.nof_tb_crc_bits == 16 ? 16 : 0x24A);
  dec.nof_llr         = d.full_length;
  dec.max_iterations  = cfg.max_iterations;
  dec.scaling_factor  = 0.8F; // ldpc_decoder::configuration::algorithm_details default, which pusch_codeblock_decoder keeps
  return dec;
}
} // namespace

bool pusch_decoder_harq_sizes(const nrphy_pusch_decoder_cfg_t& cfg, uint32_t n_tb, uint64_t* soft_bytes_per_tb, uint64_t* state_bytes,
                              uint32_t* nof_codeblocks)
{
  PuschLayout l;
  if (!pusch_layout(cfg, n_tb, l)) {
    return false;
  }
  *soft_bytes_per_tb = (uint64_t)l.d.nof_codeblocks * l.d.full_length;
  *state_bytes       = l.state_bytes;
  *nof_codeblocks    = l.d.nof_codeblocks;
  return true;
}

extern "C" int nrphy_pusch_decoder_prepare(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg)
{
  PuschLayout l;
  if (ctx == nullptr || cfg == nullptr || !pusch_layout(*cfg, 1, l)) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, l.d);
  const int                      rc  = nrphy_ldpc_decoder_prepare(ctx, &dec);
  if (rc != NRPHY_OK) {
    return rc;
  }
  if (l.d.nof_codeblocks > 1 && get_pusch_tb_crc_weights(ctx, cfg->tb_size_bytes) == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_decoder_sizes(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb,
                                         uint64_t* soft_bytes_per_tb, uint64_t* state_bytes, uint64_t* scratch_bytes,
                                         uint32_t* nof_codeblocks)
{
  PuschLayout l;
  if (ctx == nullptr || cfg == nullptr || !pusch_layout(*cfg, n_tb, l)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (scratch_bytes) {
    const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, l.d);
    if (nrphy_ldpc_decoder_scratch_bytes(ctx, &dec, std::max<uint32_t>(1, n_tb * l.d.nof_codeblocks), scratch_bytes) != NRPHY_OK) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  if (soft_bytes_per_tb) {
    *soft_bytes_per_tb = (uint64_t)l.d.nof_codeblocks * l.d.full_length;
  }
  if (state_bytes) {
    *state_bytes = l.state_bytes;
  }
  if (nof_codeblocks) {
    *nof_codeblocks = l.d.nof_codeblocks;
  }
  return NRPHY_OK;
}

int pusch_decode_variants(nrphy_ctx_t* ctx, const PuschDecodeVariant* variants, uint32_t nof_variants, const uint32_t* d_select,
                          uint32_t n_tb, uint64_t llr_stride_bytes, int8_t* d_soft, uint8_t* d_state, void* d_scratch, uint8_t* d_tb,
                          uint32_t tb_stride_bytes, uint32_t* d_result, void* stream)
{
  const TraceRange trace("process_pusch");
  PuschLayout l;
  if (ctx == nullptr || variants == nullptr || nof_variants == 0 || (d_select == nullptr && nof_variants != 1) ||
      variants[0].cfg == nullptr || d_soft == nullptr || d_state == nullptr || d_tb == nullptr || d_scratch == nullptr ||
      d_result == nullptr || !pusch_layout(*variants[0].cfg, n_tb, l) || tb_stride_bytes < variants[0].cfg->tb_size_bytes) {
    return NRPHY_ERR_ARGUMENT;
  }
  const nrphy_pusch_decoder_cfg_t* cfg = variants[0].cfg;
  // Every variant is the same transport block in the same soft buffers: only the rate-matched lengths may differ.
  std::vector<PuschLayout> layouts(nof_variants, l);
  for (uint32_t v = 0; v != nof_variants; ++v) {
    const nrphy_pusch_decoder_cfg_t* c = variants[v].cfg;
    if (c == nullptr || variants[v].d_llr == nullptr || !pusch_layout(*c, n_tb, layouts[v]) ||
        llr_stride_bytes < (uint64_t)c->nof_ch_symbols * c->qm || c->base_graph != cfg->base_graph || c->qm != cfg->qm ||
        c->rv != cfg->rv || c->nof_layers != cfg->nof_layers || c->nref != cfg->nref || c->tb_size_bytes != cfg->tb_size_bytes ||
        c->max_iterations != cfg->max_iterations || c->use_early_stop != cfg->use_early_stop || c->new_data != cfg->new_data ||
        layouts[v].state_bytes != l.state_bytes || layouts[v].d.full_length != l.d.full_length ||
        layouts[v].d.nof_codeblocks != l.d.nof_codeblocks || layouts[v].d.nof_filler_bits != l.d.nof_filler_bits) {
      return NRPHY_ERR_ARGUMENT;
    }
  }
  if (n_tb == 0) {
    return NRPHY_OK;
  }
  const nrphy_pdsch_derived_t& d = l.d;
  const uint32_t               C = d.nof_codeblocks, N = d.full_length;
  const uint64_t               n_cb = (uint64_t)n_tb * C;
  hipStream_t                  s    = stream ? (hipStream_t)stream : ctx->stream;
  uint8_t *                    ok = d_state + l.off_ok, *skip = d_state + l.off_skip, *msg = d_state + l.off_msg;
  uint32_t*                    iter = (uint32_t*)(d_state + l.off_iter);
  HIP_TRY(hipSetDevice(ctx->device));
  if (cfg->new_data) { // a fresh soft buffer has no codeblock CRC flags
    HIP_TRY(hipMemsetAsync(ok, 0, n_cb, s));
  }
  HIP_TRY(hipMemcpyAsync(skip, ok, n_cb, hipMemcpyDeviceToDevice, s));
  // Rate dematching of every codeblock, also of those decoded earlier (pusch_decoder_impl.cpp:340-350): the short
  // segments, then the long ones.  With variants, the launches of each; the soft buffers see those of the selected one only.
  nrphy_ldpc_rate_dematcher_cfg_t dm;
  dm.base_graph      = cfg->base_graph;
  dm.lifting_size    = d.lifting_size;
  dm.rv              = cfg->rv;
  dm.qm              = cfg->qm;
  dm.nref            = d.n_ref;
  dm.nof_filler_bits = d.nof_filler_bits;
  int rc = NRPHY_OK;
  for (uint32_t v = 0; v != nof_variants && rc == NRPHY_OK; ++v) {
    const nrphy_pdsch_derived_t& dv      = layouts[v].d;
    const int8_t*                d_llr   = variants[v].d_llr;
    const uint32_t               n_short = dv.nof_short_segments;
    if (n_short != 0) {
      dm.rm_length = dv.rm_length_short;
      rc = rate_dematch_batch(ctx, &dm, n_short, n_tb, d_llr, dv.rm_length_short, llr_stride_bytes, d_soft, N, (size_t)C * N,
                              cfg->new_data, s, d_select, variants[v].select_value);
    }
    if (rc == NRPHY_OK && n_short != C) {
      dm.rm_length = dv.rm_length_long;
      rc = rate_dematch_batch(ctx, &dm, C - n_short, n_tb, d_llr + (size_t)n_short * dv.rm_length_short, dv.rm_length_long,
                              llr_stride_bytes, d_soft + (size_t)n_short * N, N, (size_t)C * N, cfg->new_data, s, d_select,
                              variants[v].select_value);
    }
  }
  if (rc != NRPHY_OK) {
    return rc;
  }
  const nrphy_ldpc_decoder_cfg_t dec = pusch_ldpc_cfg(*cfg, d);
  // How far into the soft buffers a first transmission reaches (filler bits included): what the decoder can expect to be in
  // use when the buffers held nothing else -- a hint for the launch's LDS size only (see ldpc_decode_batch).
  uint32_t expected_extent = 0;
  if (cfg->new_data) {
    const unsigned bg_k = (cfg->base_graph == 1) ? 22 : 10, zc = d.lifting_size;
    const unsigned buffer_length = (d.n_ref > 0 && d.n_ref < N) ? d.n_ref : N;
    static const double shift_bg1[4] = {0, 17, 33, 56}, shift_bg2[4] = {0, 13, 25, 43};
    const double   frac = (((cfg->base_graph == 1) ? shift_bg1 : shift_bg2)[cfg->rv] * buffer_length) / N;
    const unsigned k0   = (unsigned)((uint16_t)std::floor(frac)) * zc;
    std::vector<DematchOp> ops;
    std::vector<uint32_t> lengths; // of every variant: the hint takes the largest extent
    for (const PuschLayout& lv : layouts) {
      lengths.push_back(lv.d.rm_length_short);
      lengths.push_back(lv.d.rm_length_long);
    }
    for (uint32_t e : lengths) {
      if (e == 0) {
        continue;
      }
      build_dematch_ops(ops, N, buffer_length, k0, (bg_k - 2) * zc, d.nof_filler_bits, e, true);
      for (const DematchOp& op : ops) {
        if (op.kind != DEMATCH_ZERO) {
          expected_extent = std::max<uint32_t>(expected_extent, op.begin + op.count);
        }
      }
    }
  }
  rc = ldpc_decode_batch(ctx, &dec, (uint32_t)n_cb, d_soft, N, msg, l.msg_stride, iter, skip, ok, cfg->use_early_stop == 0,
                         d_scratch, s, expected_extent);
  if (rc != NRPHY_OK) {
    return rc;
  }
  PuschAssembleLaunch a;
  a.crc_weight = nullptr;
  if (C > 1) {
    a.crc_weight = get_pusch_tb_crc_weights(ctx, cfg->tb_size_bytes); // uploaded by nrphy_pusch_decoder_prepare() or here
    if (a.crc_weight == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
  }
  a.cb_msg         = msg;
  a.cb_ok          = ok;
  a.cb_iter        = iter;
  a.skipped        = skip;
  a.tb             = d_tb;
  a.result         = d_result;
  a.C              = C;
  a.msg_stride     = l.msg_stride;
  a.tb_stride      = tb_stride_bytes;
  a.tb_bytes       = cfg->tb_size_bytes;
  a.cb_info_bits   = d.cb_info_bits;
  a.max_iterations = cfg->max_iterations;
  // The transport-block check by 16 KiB regions (tbcrc_regions_workgroup, the transmit side's TB-CRC role): the context's
  // tables and the factor that turns the remainder of the zero-extended block into the block's CRC24A.
  a.tbcrc          = ctx->d_tbcrc;
  a.crc_factor     = CRC24A_FIELD.xpow((int64_t)CRC24A_FIELD.order +
                                   8 * ((int64_t)cfg->tb_size_bytes -
                                        (int64_t)divide_ceil(cfg->tb_size_bytes, TB_CRC_REGION_BYTES) * TB_CRC_REGION_BYTES));
  HIP_TRY(launch_pusch_assemble(a, n_tb, s));
  return NRPHY_OK;
}

extern "C" int nrphy_pusch_decode_batch(nrphy_ctx_t* ctx, const nrphy_pusch_decoder_cfg_t* cfg, uint32_t n_tb,
                                        const int8_t* d_llr, uint64_t llr_stride_bytes, int8_t* d_soft, uint8_t* d_state,
                                        void* d_scratch, uint8_t* d_tb, uint32_t tb_stride_bytes, uint32_t* d_result, void* stream)
{
  const PuschDecodeVariant one = {cfg, d_llr, 0};
  return pusch_decode_variants(ctx, &one, 1, nullptr, n_tb, llr_stride_bytes, d_soft, d_state, d_scratch, d_tb, tb_stride_bytes,
                               d_result, stream);
}
