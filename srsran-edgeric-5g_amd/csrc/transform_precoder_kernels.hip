// Transform deprecoder for gfx950, stand-alone form.
//
// Replaces transform_precoder::deprecode_ofdm_symbol (R/lib/phy/generic_functions/transform_precoding/
// transform_precoder_dft_impl.cpp:31-57): an unnormalised inverse DFT of M_sc = 12 * M_rb points, then a multiplication by the
// float 1 / sqrt(M_sc).  One workgroup per OFDM symbol: the symbol into LDS, mixed_dft_inverse() (dft_mixed_device.h, the routine
// the fused PUSCH demodulator runs), the scaled result out.  A workgroup has read its whole symbol before it writes, so the
// output may be the input.
#include "dft_mixed_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

__global__ __launch_bounds__(MIXED_DFT_THREADS) void transform_deprecode_kernel(MixedDftPlan p, const float2* in, float2* out)
{
  __shared__ cf  buf[2][MIXED_DFT_MAX_POINTS];
  const uint32_t tid  = threadIdx.x;
  const size_t   base = (size_t)blockIdx.x * p.n;
  for (uint32_t i = tid; i < p.n; i += MIXED_DFT_THREADS) {
    const float2 v = in[base + i];
    buf[0][i]      = make_cf(v.x, v.y);
  }
  const cf* z = mixed_dft_inverse(p, buf[0], buf[1], tid);
  for (uint32_t i = tid; i < p.n; i += MIXED_DFT_THREADS) {
    const cf v    = z[i];
    out[base + i] = make_float2(__fmul_rn(v.x, p.scale), __fmul_rn(v.y, p.scale));
  }
}

} // namespace

hipError_t launch_transform_deprecode(const MixedDftPlan& plan, uint32_t batch, const float2* in, float2* out, hipStream_t stream)
{
  if (batch == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(transform_deprecode_kernel, dim3(batch), dim3(MIXED_DFT_THREADS), 0, stream, plan, in, out);
  return hipGetLastError();
}

} // namespace nrphy
