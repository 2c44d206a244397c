// PUSCH DM-RS channel estimator for gfx950.
//
// Replaces dmrs_pusch_estimator_impl::estimate (R/lib/phy/upper/signal_processors/dmrs_pusch_estimator_impl.cpp:71-212) with
// port_channel_estimator_average_impl::compute (port_channel_estimator_average_impl.cpp, filter smoothing and CFO compensation
// on) and the DC step of pusch_processor_impl (pusch_processor_impl.cpp:182-199).  DM-RS type 1, one or two layers.
//
// Two kernels (plan built on the host, pusch_chest_host.cpp):
//  (A) pusch_chest_kernel<source>: one 256-thread workgroup per (PUSCH, receive port, layer).  Pilots from the Gold sequence
//      (gold_sequence_wave, one DM-RS symbol per wave) or, for a transform-precoded PUSCH, the low-PAPR sequence of
//      TS 38.211 Section 6.4.1.1.1.2 (low_papr_device.h): one 16-bit circle index per pilot, computed once per workgroup into the
//      LDS the Gold words would take and turned into the phasor at each use.  The source is a template parameter
//      (pusch_chest_kernel_device.h), one instantiation each -- the Gold one here, the low-PAPR one in
//      pusch_chest_lowpapr_kernels.hip --, one launch per job group; everything behind pilot() is shared.  LS estimates, EPRE,
//      CFO from the first two DM-RS symbols, CFO derotation and averaging; virtual pilots and the raised-cosine FIR in LDS; RSRP, noise and SNR; the time alignment as a
//      direct 288-bin partial inverse DFT; the linear interpolation (the reference's running sum, one lane per component),
//      rounded to cbf16 into the plan's scratch row, and the per-symbol CFO rotations.  Every reduction is a per-thread
//      double partial sum folded in a fixed order: two runs give the same bits.
//  (B) pusch_chest_expand_kernel: one workgroup per (job, OFDM symbol): the scratch row rotated by the symbol's CFO phasor and
//      rounded again (the reference rounds twice), DC zeroed, written to the allocated PRBs with 16-byte stores.
// Transcendentals (atan2, hypot, cos, sin) are evaluated in double and rounded once to float.  Contraction is off; the only
// fused multiply-adds are the partial DFT's, which feed a comparison and nothing else.  The virtual pilots and the
// measurements' arithmetic are chest_device.h's, shared with the PUCCH format 2 receiver; the products, the phasor, the pilot
// and the search's comparison are exact_device.h's, shared with every receiver.
#include "pusch_chest_kernel_device.h"

namespace nrphy {
namespace {

// One workgroup per (job, OFDM symbol): 16-byte chunks of 4 RE, 3 per PRB.
__global__ __launch_bounds__(CHEST_THREADS) void pusch_chest_expand_kernel(PuschChestLaunch p)
{
  const uint32_t        j = blockIdx.x, l = blockIdx.y;
  const uint32_t        job = p.jobs[j];
  const uint32_t        ip = job >> 8, port = (job >> 4) & 15u, layer = job & 15u;
  const PuschChestDesc& d = p.desc[ip];
  if (l < d.first_symbol || l >= d.first_symbol + d.nof_symbols) {
    return;
  }
  const uint32_t* src = p.rows + d.row_offset + (size_t)(port * d.nof_layers + layer) * 12u * d.nprb;
  uint32_t*       dst = p.ch + d.ce_offset + (((size_t)layer * d.nof_rx_ports + port) * NRPHY_NSYMB + l) * p.grid_nof_subc;
  const bool      rot = d.nof_dmrs >= 2u, wide = (((uintptr_t)dst) & 15u) == 0; // rows of a PUSCH share their phase
  const float2    r   = p.rot[(size_t)j * NRPHY_NSYMB + l];
  for (uint32_t c = threadIdx.x; c < 3u * d.nprb; c += CHEST_THREADS) {
    uint4          w  = reinterpret_cast<const uint4*>(src)[c];
    const uint32_t k0 = 12u * p.prbs[d.prb_first + c / 3u] + 4u * (c % 3u);
    uint32_t*      v  = &w.x;
#pragma unroll
    for (uint32_t i = 0; i != 4; ++i) {
      if (rot) {
        const float2 e = exact::cmul(cbf16_to_float2(v[i]), r);
        v[i]           = to_cbf16(e.x, e.y);
      }
      if (k0 + i == d.dc) {
        v[i] = 0u;
      }
    }
    if (wide) {
      reinterpret_cast<uint4*>(dst + k0)[0] = w;
    } else {
      dst[k0] = w.x;
      dst[k0 + 1u] = w.y;
      dst[k0 + 2u] = w.z;
      dst[k0 + 3u] = w.w;
    }
  }
}

} // namespace

hipError_t launch_pusch_chest(const PuschChestLaunch& p, uint32_t n_gold, hipStream_t stream)
{
  if (p.n_jobs == 0 || n_gold > p.n_jobs) {
    return p.n_jobs == 0 ? hipSuccess : hipErrorInvalidValue;
  }
  if (n_gold != 0) {
    hipLaunchKernelGGL(pusch_chest_kernel<PILOT_GOLD>, dim3(n_gold), dim3(CHEST_THREADS), 0, stream, p);
  }
  if (n_gold != p.n_jobs) { // the job group behind the Gold one: its jobs and its rows of the rotations
    PuschChestLaunch lp = p;
    lp.jobs += n_gold;
    lp.rot += (size_t)n_gold * NRPHY_NSYMB;
    lp.n_jobs = p.n_jobs - n_gold;
    launch_pusch_chest_lowpapr(lp, stream);
  }
  hipLaunchKernelGGL(pusch_chest_expand_kernel, dim3(p.n_jobs, NRPHY_NSYMB), dim3(CHEST_THREADS), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
