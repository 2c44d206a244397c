// Host side of ldpc_dematcher.hip: the rate dematcher's list of range operations and its launch.
#include "ldpc_receive_host.h"

#include <cmath>

void build_dematch_ops(std::vector<DematchOp>& ops, unsigned block_length, unsigned buffer_length, unsigned k0,
                       unsigned nof_systematic, unsigned nof_filler, unsigned e, bool new_data)
{
  const unsigned nof_info = nof_systematic - nof_filler;
  bool           copying  = new_data;
  unsigned       pos = k0, taken = 0;
  ops.clear();
  auto emit = [&](uint32_t kind, unsigned begin, unsigned count, unsigned src) {
    if (count != 0) {
      ops.push_back({kind, begin, count, src});
    }
  };
  while (taken != e) {
    unsigned left = e - taken;
    if (pos < nof_info) {
      const unsigned n = std::min(nof_info - pos, left);
      if (copying) {
        emit(DEMATCH_ZERO, 0, pos, 0);
      }
      emit(copying ? DEMATCH_COPY : DEMATCH_COMBINE, pos, n, taken);
      pos += n;
      taken += n;
      left -= n;
    } else if (copying) {
      emit(DEMATCH_ZERO, 0, nof_info, 0);
    }
    if (copying) {
      emit(DEMATCH_FILL, nof_info, nof_filler, 0);
    }
    pos = std::max(pos, nof_systematic);
    const unsigned n = std::min(buffer_length - pos, left);
    emit(copying ? DEMATCH_COPY : DEMATCH_COMBINE, pos, n, taken);
    pos = (pos + n) % buffer_length;
    taken += n;
    if (taken != e) {
      copying = false;
    }
  }
  if (copying && pos != 0) {
    // the reference clears this many soft bits at the end of the full-length block, wherever the buffer ends
    emit(DEMATCH_ZERO, block_length - (buffer_length - pos), buffer_length - pos, 0);
  }
}

int rate_dematch_batch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb, uint32_t n_outer,
                       const int8_t* d_in, uint32_t in_stride_bytes, size_t in_outer, int8_t* d_soft,
                       uint32_t soft_stride_bytes, size_t soft_outer, int new_data, void* stream, const uint32_t* d_select,
                       uint32_t select_value)
{
  if (ctx == nullptr || cfg == nullptr || d_in == nullptr || d_soft == nullptr ||
      (cfg->base_graph != 1 && cfg->base_graph != 2) || cfg->rv > 3 || lifting_position(cfg->lifting_size) < 0 ||
      (cfg->qm != 1 && cfg->qm != 2 && cfg->qm != 4 && cfg->qm != 6 && cfg->qm != 8) || cfg->rm_length == 0 ||
      cfg->rm_length > 35 * 8448 /* ldpc::MAX_CODEBLOCK_RM_SIZE */ || cfg->rm_length % cfg->qm != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  static const double shift_bg1[4] = {0, 17, 33, 56}, shift_bg2[4] = {0, 13, 25, 43};
  const unsigned      zc = cfg->lifting_size, n_short = (cfg->base_graph == 1) ? 66 : 50;
  const unsigned      block_length   = n_short * zc;
  const unsigned      buffer_length  = (cfg->nref > 0 && cfg->nref < block_length) ? cfg->nref : block_length;
  const unsigned      nof_systematic = (((cfg->base_graph == 1) ? 22 : 10) - 2) * zc;
  if (cfg->nof_filler_bits >= nof_systematic || buffer_length <= nof_systematic || in_stride_bytes < cfg->rm_length ||
      soft_stride_bytes < block_length) {
    return NRPHY_ERR_ARGUMENT;
  }
  // ldpc_rate_dematcher_impl.cpp:94-95: k0 of TS 38.212 Table 5.4.2.1-2 in double precision
  const double   frac = (((cfg->base_graph == 1) ? shift_bg1 : shift_bg2)[cfg->rv] * buffer_length) / block_length;
  const unsigned k0   = (unsigned)((uint16_t)std::floor(frac)) * zc;
  DematchLaunch          p;
  std::vector<DematchOp> ops;
  build_dematch_ops(ops, block_length, buffer_length, k0, nof_systematic, cfg->nof_filler_bits, cfg->rm_length,
                    new_data != 0);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t   s = stream ? (hipStream_t)stream : ctx->stream;
  StreamStaging staging(s);
  p.n_ops   = (uint32_t)ops.size();
  p.ops_ext = nullptr;
  if (ops.size() <= MAX_DEMATCH_OPS) {
    std::copy(ops.begin(), ops.end(), p.ops);
  } else {
    // Heavy repetition (rm_length of dozens of buffer lengths): the list goes through device memory of this call's
    // own, allocated, filled and released in stream order.
    DematchOp* d_ops = (DematchOp*)staging.alloc(ops.size() * sizeof(DematchOp));
    if (d_ops == nullptr) {
      return NRPHY_ERR_DEVICE;
    }
    HIP_TRY(hipMemcpyAsync(d_ops, ops.data(), ops.size() * sizeof(DematchOp), hipMemcpyHostToDevice, s));
    p.ops_ext = d_ops;
  }
  {
    // Do the copying / clearing / filling operations cover the whole block?  Then no soft bit keeps its old value and the
    // kernel skips reading the buffer (always so for a first transmission that does not wrap; never with combining).
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    bool combines = false;
    for (const DematchOp& op : ops) {
      combines = combines || op.kind == DEMATCH_COMBINE;
      ranges.emplace_back(op.begin, op.begin + op.count);
    }
    std::sort(ranges.begin(), ranges.end());
    uint32_t reach = 0;
    for (const auto& r : ranges) {
      if (r.first > reach) {
        break;
      }
      reach = std::max(reach, r.second);
    }
    p.skip_load = (!combines && reach >= block_length) ? 1U : 0U;
    // Pairwise disjoint destination ranges (sorted by begin: each starts where the previous one has ended or later)?
    p.disjoint = 1U;
    for (size_t i = 1; i < ranges.size(); ++i) {
      if (ranges[i].first < ranges[i - 1].second) {
        p.disjoint = 0U;
      }
    }
  }
  p.select       = d_select;
  p.select_value = select_value;
  p.in           = d_in;
  p.out          = d_soft;
  p.in_stride    = in_stride_bytes;
  p.out_stride   = soft_stride_bytes;
  p.block_length = block_length;
  p.qm           = cfg->qm;
  p.cols         = cfg->rm_length / cfg->qm;
  p.in_stride_outer  = (uint32_t)in_outer;
  p.out_stride_outer = (uint32_t)soft_outer;
  if (in_outer > 0xFFFFFFFFULL || soft_outer > 0xFFFFFFFFULL) {
    return NRPHY_ERR_CAPACITY;
  }
  HIP_TRY(launch_ldpc_dematch(p, n_cb, s, n_outer));
  return NRPHY_OK;
}

extern "C" int nrphy_ldpc_rate_dematch(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg, uint32_t n_cb,
                                       const int8_t* d_in, uint32_t in_stride_bytes, int8_t* d_soft,
                                       uint32_t soft_stride_bytes, int new_data, void* stream)
{
  return rate_dematch_batch(ctx, cfg, n_cb, 1, d_in, in_stride_bytes, 0, d_soft, soft_stride_bytes, 0, new_data, stream);
}

extern "C" int nrphy_ldpc_rate_dematch_host(nrphy_ctx_t* ctx, const nrphy_ldpc_rate_dematcher_cfg_t* cfg,
                                            const int8_t* in, int8_t* soft_buffer, int new_data)
{
  // Everything that sizes a copy below is checked here, before the validating device-pointer call runs.
  if (ctx == nullptr || cfg == nullptr || in == nullptr || soft_buffer == nullptr ||
      (cfg->base_graph != 1 && cfg->base_graph != 2) || lifting_position(cfg->lifting_size) < 0 || cfg->rm_length == 0 ||
      cfg->rm_length > 35 * 8448) {
    return NRPHY_ERR_ARGUMENT;
  }
  const unsigned block_length = ((cfg->base_graph == 1) ? 66U : 50U) * cfg->lifting_size;
  HostCall       call(ctx);
  uint8_t*       d[2]; // in, soft buffer
  if (!call.carve(SCRATCH_RX, {(size_t)cfg->rm_length + 16, (size_t)block_length + 16}, d)) {
    return NRPHY_ERR_DEVICE;
  }
  int8_t *d_in = (int8_t*)d[0], *d_soft = (int8_t*)d[1];
  HIP_TRY(hipMemcpy(d_in, in, cfg->rm_length, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_soft, soft_buffer, block_length, hipMemcpyHostToDevice));
  const int rc = nrphy_ldpc_rate_dematch(ctx, cfg, 1, d_in, cfg->rm_length, d_soft, block_length, new_data, ctx->stream);
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(soft_buffer, d_soft, block_length, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}
