// The low-PAPR instantiation of the PUSCH DM-RS channel estimator's first kernel (pusch_chest_kernel_device.h; the plan, the Gold
// instantiation and the expand kernel are pusch_chest_kernels.hip's), and the kernel that writes the sequence alone.
#include "pusch_chest_kernel_device.h"

namespace nrphy {
namespace {

__global__ __launch_bounds__(CHEST_THREADS) void pusch_lowpapr_sequence_kernel(const PuschChestDesc* desc, float2* out)
{
  const PuschChestDesc& d = desc[0];
  const uint32_t        n = blockIdx.x * CHEST_THREADS + threadIdx.x;
  if (n < 6u * d.nprb) {
    out[n] = unit_circle_libm(low_papr_dmrs_index(d, n), d.lp.circle);
  }
}


} // namespace

void launch_pusch_chest_lowpapr(const PuschChestLaunch& p, hipStream_t stream)
{
  hipLaunchKernelGGL(pusch_chest_kernel<PILOT_LOW_PAPR>, dim3(p.n_jobs), dim3(CHEST_THREADS), 0, stream, p);
}

hipError_t launch_pusch_lowpapr_sequence(const PuschChestDesc* desc, float2* out, hipStream_t stream)
{
  hipLaunchKernelGGL(pusch_lowpapr_sequence_kernel, dim3((MAX_PILOTS + CHEST_THREADS - 1) / CHEST_THREADS), dim3(CHEST_THREADS), 0, stream,
                     desc, out);
  return hipGetLastError();
}

} // namespace nrphy
