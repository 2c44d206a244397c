// PUSCH processor with CSI part 2 for gfx950: the select kernel and the part 2 result kernel of nrphy_pusch_csi2_run.
//
// The plan has enumerated every size a PDU's part 2 can take and derived a finished configuration for each (a "variant"); what is
// left for the device is to find out which one the UE sent.  The select kernel replaces pusch_processor_impl's feedback step
// (pusch_processor_impl.cpp:57-86 with uci_part2_get_size, R/lib/ran/uci/uci_part2_size_calculator.cpp): it runs behind the UCI
// decoder of HARQ-ACK and CSI part 1, evaluates the PDU's size description on the decoded part 1 payload, looks the size up in the
// PDU's variant table and writes the PDU's select word -- 0, "no part 2", when part 1 did not decode `valid` or the size is 0.  The
// demultiplexer, UCI decoder and rate-dematcher launches behind it hold every variant; their workgroups compare the word with their
// own value and all but the selected ones return.  It also clears the statuses of the PDU's part 2 messages, of which at most the
// selected one is written again in this run.
//
// The work per PDU is a handful of bytes, so the split is the result kernel's of pusch_proc_kernels.hip: one wavefront per PDU, four
// per workgroup, no LDS, no barrier, no atomics.  The PDU index is made scalar (readfirstlane), so the descriptor, the status and
// the branches on them are wave-uniform; every lane evaluates the description (at most eight payload bytes, the same addresses in
// every lane), lane v compares the size with row v of the table, a ballot gives the row, and the stores are plain vector stores:
// lane 0 the select word, lanes 1 .. nof_variants - 1 a status each.
#include "bits_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t CSI2_WAVES = 4; // PDUs per workgroup

__global__ __launch_bounds__(CSI2_WAVES * WAVE) void pusch_csi2_select_kernel(PuschCsi2Launch p)
{
  const uint32_t ip = __builtin_amdgcn_readfirstlane(blockIdx.x * CSI2_WAVES + (threadIdx.x >> 6));
  if (ip >= p.n) {
    return;
  }
  const PuschCsi2Desc& d    = p.desc[ip];
  const uint32_t       lane = threadIdx.x & 63u;
  uint32_t             size = 0;
  if (d.nof_entries != 0 && p.status[d.csi1_status] == NRPHY_UCI_STATUS_VALID) { // wave-uniform
    const uint8_t* bits = p.uci_bits + d.csi1_offset;
    for (uint32_t e = 0; e != d.nof_entries; ++e) {
      uint32_t index = 0;
      for (uint32_t k = 0; k != d.nof_parameters[e]; ++k) {
        uint32_t value = 0;
        for (uint32_t j = 0; j != d.width[e][k]; ++j) { // the payload bit at `offset` is the value's most significant bit
          value |= (uint32_t)(bits[d.offset[e][k] + j] & 1u) << (d.width[e][k] - 1u - j);
        }
        index = (index << d.width[e][k]) | value;
      }
      size += d.map[e][index & ((1u << NRPHY_PUSCH_CSI2_MAX_ENTRY_BITS) - 1u)];
    }
  }
  // Row 0 is size 0; the plan enumerated every sum of map values, so a size above 0 has exactly one row.
  const bool     mine    = lane != 0 && lane < d.nof_variants && d.size[lane] == size;
  const uint64_t rows    = __ballot(mine);
  const uint32_t variant = rows != 0 ? (uint32_t)__ffsll((unsigned long long)rows) - 1u : 0u;
  if (lane == 0) {
    p.select[ip] = variant;
  } else if (lane < d.nof_variants) {
    p.variant_status[d.status_base + lane - 1u] = NRPHY_UCI_STATUS_UNKNOWN;
  }
}

// Behind every stage: one record per PDU, written once by lane 0 of the PDU's wavefront.
__global__ __launch_bounds__(CSI2_WAVES * WAVE) void pusch_csi2_result_kernel(PuschCsi2Launch p)
{
  const uint32_t ip = __builtin_amdgcn_readfirstlane(blockIdx.x * CSI2_WAVES + (threadIdx.x >> 6));
  if (ip >= p.n || (threadIdx.x & 63u) != 0) {
    return;
  }
  const PuschCsi2Desc& d = p.desc[ip];
  const uint32_t       v = p.select[ip] < d.nof_variants ? p.select[ip] : 0u;
  nrphy_pusch_csi2_result_t r;
  r.status           = v != 0 ? p.variant_status[d.status_base + v - 1u] : NRPHY_UCI_STATUS_UNKNOWN;
  r.nof_csi_part2    = d.size[v];
  r.csi_part2_offset = v != 0 ? d.csi2_offset : 0u;
  r.nof_enc_bits     = d.nof_enc[v];
  r.nof_ul_sch_bits  = d.nof_ul_sch[v];
  r.variant          = v;
  r.reserved_        = 0;
  p.result[ip]       = r;
}

} // namespace

hipError_t launch_pusch_csi2_select(const PuschCsi2Launch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pusch_csi2_select_kernel, dim3((p.n + CSI2_WAVES - 1) / CSI2_WAVES), dim3(CSI2_WAVES * WAVE), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_pusch_csi2_result(const PuschCsi2Launch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pusch_csi2_result_kernel, dim3((p.n + CSI2_WAVES - 1) / CSI2_WAVES), dim3(CSI2_WAVES * WAVE), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
