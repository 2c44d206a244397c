// PUSCH processor for gfx950: the result kernel, the last launch of nrphy_pusch_proc_run.
//
// Replaces what pusch_processor_impl::process and its notifier adaptor put together for the MAC once the stages have run
// (R/lib/phy/upper/channel_processors/pusch/pusch_processor_impl.cpp:200-202, pusch_processor_notifier_adaptor.h:154-163):
// channel_estimate::get_channel_state_information (R/include/srsran/phy/upper/channel_estimation.h:250-288) over layer 0 of the
// PDU's receive ports, with get_layer_average_snr (channel_estimation.h:162-179), the demodulator's post-equalisation SINR merged
// in, and the verdicts of the transport-block and UCI decoders.
//
// A record is made of at most four 32-byte measurement rows, four decoder words, two statuses and one float, so the split is the
// PUCCH receivers': one wavefront per PDU, four per workgroup, no LDS, no barrier, no atomics, no scratch.  The PDU index is made
// scalar (readfirstlane), so the descriptor is read with scalar loads.  Every lane issues at most two 16-byte loads -- lanes 0..3
// a port's row, lane 4 the decoder words, lanes 5..7 the SINR (with the EVM, where the plan takes one) and the statuses --, the values are handed round with shuffles, the
// sums over the ports are taken in port order in float as the reference takes them, and lane 0 stores the record once.  log10 is
// evaluated in double and rounded once (to_dB and the merge, CsiMerge, are exact_device.h's).  Contraction is off.
#include "bits_device.h"
#include "exact_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t PROC_WAVES = 4; // PDUs per workgroup

__global__ __launch_bounds__(PROC_WAVES * WAVE) void pusch_proc_result_kernel(PuschProcLaunch p)
{
  const uint32_t ip = __builtin_amdgcn_readfirstlane(blockIdx.x * PROC_WAVES + (threadIdx.x >> 6));
  if (ip >= p.n) {
    return;
  }
  const PuschProcDesc& d    = p.desc[ip];
  const uint32_t       lane = threadIdx.x & 63u;
  const uint32_t       P    = d.nof_rx_ports;

  uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
  if (lane < P) { // layer 0 of receive port `lane`: noise_var, rsrp, epre, snr | ta_s, ta_bins, cfo_hz, -
    const uint4* row = reinterpret_cast<const uint4*>(p.meas + ((size_t)ip * NRPHY_MAX_PORTS + lane) * NRPHY_PUSCH_CHEST_MAX_LAYERS);
    a                = row[0];
    b                = row[1];
  } else if (lane == 4) {
    if (d.has_sch != 0) {
      a = reinterpret_cast<const uint4*>(p.dec)[ip];
    }
  } else if (lane == 5) {
    a.x = __float_as_uint(p.sinr_db[ip]);
    if (d.has_evm != 0) {
      a.y = __float_as_uint(p.evm[ip]);
    }
  } else if (lane == 6) {
    a.x = d.harq_status != PUSCH_PROC_NO_STATUS ? p.status[d.harq_status] : NRPHY_UCI_STATUS_UNKNOWN;
  } else if (lane == 7) {
    a.x = d.csi1_status != PUSCH_PROC_NO_STATUS ? p.status[d.csi1_status] : NRPHY_UCI_STATUS_UNKNOWN;
  }

  CsiMerge csi;
#pragma unroll
  for (uint32_t q = 0; q != NRPHY_MAX_PORTS; ++q) {
    const float noise = __uint_as_float(__shfl(a.x, q)), rsrp = __uint_as_float(__shfl(a.y, q));
    const float epre = __uint_as_float(__shfl(a.z, q)), snr = __uint_as_float(__shfl(a.w, q));
    const float ta = __uint_as_float(__shfl(b.x, q)), cfo = __uint_as_float(__shfl(b.z, q));
    if (q < P) {
      csi.add(q, noise, rsrp, epre, snr, ta, cfo);
    }
  }
  const uint32_t dec0 = __shfl(a.x, 4), dec1 = __shfl(a.y, 4), dec2 = __shfl(a.z, 4), dec3 = __shfl(a.w, 4);
  const float    sinr_post_eq = __uint_as_float(__shfl(a.x, 5)), evm = __uint_as_float(__shfl(a.y, 5));
  const uint32_t harq_status = __shfl(a.x, 6), csi1_status = __shfl(a.x, 7);
  if (lane != 0) {
    return;
  }
  const float sinr_ce = csi.sinr_dB();
  const bool  has_cfo = csi.cfo_hz == csi.cfo_hz; // the estimator reports NaN where the reference's optional is empty

  nrphy_pusch_result_t r;
  r.has_sch              = d.has_sch;
  r.tb_crc_ok            = dec0;
  r.nof_codeblocks       = d.has_sch != 0 ? d.nof_codeblocks : 0u;
  r.nof_codeblocks_ok    = dec1;
  r.ldpc_iterations_sum  = dec2;
  r.ldpc_iterations_max  = dec3;
  r.harq_ack_status      = harq_status;
  r.csi_part1_status     = csi1_status;
  r.nof_harq_ack         = d.nof_harq_ack;
  r.nof_csi_part1        = d.nof_csi_part1;
  r.harq_ack_offset      = d.harq_ack_offset;
  r.csi_part1_offset     = d.csi_part1_offset;
  r.sinr_ch_estimator_dB = sinr_ce;
  r.sinr_post_eq_dB      = sinr_post_eq;
  r.sinr_dB              = d.sinr_method == NRPHY_PUSCH_SINR_POST_EQUALIZATION ? sinr_post_eq : sinr_ce;
  if (d.sinr_method == NRPHY_PUSCH_SINR_EVM) { // pusch_processor_notifier_adaptor.h:157-162, in float as there
    r.sinr_dB = evm == 0.f ? F_INF : __fsub_rn(__fmul_rn(-20.0f, log10f(evm)), 3.7f);
  }
  r.epre_dB              = csi.epre_dB(P);
  r.rsrp_dB              = csi.rsrp_dB(P);
  r.time_alignment_s     = csi.ta_s;
  r.cfo_hz               = has_cfo ? csi.cfo_hz : 0.f;
  r.has_cfo              = has_cfo ? 1u : 0u;
  r.has_evm              = d.has_evm;
  r.evm                  = evm; // 0 without has_evm: lane 5 left the word as it was
  p.result[ip]           = r;
}

} // namespace

hipError_t launch_pusch_proc_result(const PuschProcLaunch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pusch_proc_result_kernel, dim3((p.n + PROC_WAVES - 1) / PROC_WAVES), dim3(PROC_WAVES * WAVE), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
