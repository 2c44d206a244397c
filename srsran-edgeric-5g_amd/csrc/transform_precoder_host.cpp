// Host side of the transform deprecoder (transform_precoder_kernels.hip, and the fused form in pusch_demod_kernels.hip): which
// sizes are valid, the stage list of a size, and the stand-alone entry points.
#include "nrphy_host_internal.h"

#include <cmath>

// transform_precoding::is_nof_prbs_valid (R/include/srsran/ran/transform_precoding/transform_precoding_helpers.h): 2^a 3^b 5^c,
// 1..275.  53 values, the largest 270.
extern "C" int nrphy_transform_precoding_nof_prb_valid(uint32_t nof_prb)
{
  if (nof_prb == 0 || nof_prb > NRPHY_MAX_RB) {
    return 0;
  }
  for (uint32_t f : {2U, 3U, 5U}) {
    while (nof_prb % f == 0) {
      nof_prb /= f;
    }
  }
  return nof_prb == 1;
}

// Radix 4 first (12 * M_rb always has one), then what is left of the factors 2, 3 and 5.
bool nrphy::mixed_dft_stages(uint32_t nof_prb, MixedDftPlan& plan)
{
  if (!nrphy_transform_precoding_nof_prb_valid(nof_prb)) {
    return false;
  }
  std::memset(&plan, 0, sizeof(plan));
  plan.n     = NRPHY_NRE * nof_prb;
  plan.scale = 1.0F / std::sqrt((float)plan.n); // transform_precoder_dft_impl.cpp:53
  uint32_t left = plan.n;
  for (uint32_t r : {4U, 2U, 3U, 5U}) {
    while (left % r == 0) {
      if (plan.nof_stages == MIXED_DFT_MAX_STAGES) {
        return false;
      }
      plan.radix[plan.nof_stages++] = (uint8_t)r;
      left /= r;
    }
  }
  return left == 1;
}

bool transform_deprecode_plan(nrphy_ctx* ctx, uint32_t nof_prb, MixedDftPlan& plan)
{
  if (!mixed_dft_stages(nof_prb, plan)) {
    return false;
  }
  plan.twiddle = get_twiddle_table(ctx, plan.n);
  return plan.twiddle != nullptr;
}

extern "C" int nrphy_transform_deprecode(nrphy_ctx_t* ctx, uint32_t nof_prb, uint32_t batch, const float* d_in, float* d_out,
                                         void* stream)
{
  MixedDftPlan plan;
  if (ctx == nullptr || !mixed_dft_stages(nof_prb, plan)) {
    return NRPHY_ERR_ARGUMENT;
  }
  if (batch == 0) {
    return NRPHY_OK;
  }
  if (d_in == nullptr || d_out == nullptr || (((uintptr_t)d_in | (uintptr_t)d_out) & 7U) != 0) {
    return NRPHY_ERR_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (!transform_deprecode_plan(ctx, nof_prb, plan)) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(launch_transform_deprecode(plan, batch, (const float2*)d_in, (float2*)d_out, stream ? (hipStream_t)stream : ctx->stream));
  return NRPHY_OK;
}

extern "C" int nrphy_transform_deprecode_host(nrphy_ctx_t* ctx, uint32_t nof_prb, const float* in, float* out)
{
  if (ctx == nullptr || in == nullptr || out == nullptr || !nrphy_transform_precoding_nof_prb_valid(nof_prb)) {
    return NRPHY_ERR_ARGUMENT;
  }
  const size_t bytes = (size_t)NRPHY_NRE * nof_prb * sizeof(float2);
  HostCall     call(ctx);
  float*       d_buf = call.mem<float>(SCRATCH_RX, bytes);
  if (d_buf == nullptr) {
    return NRPHY_ERR_DEVICE;
  }
  HIP_TRY(hipMemcpy(d_buf, in, bytes, hipMemcpyHostToDevice));
  const int rc = nrphy_transform_deprecode(ctx, nof_prb, 1, d_buf, d_buf, ctx->stream); // in place, as the reference calls it
  if (rc != NRPHY_OK) {
    return rc;
  }
  HIP_TRY(call.sync());
  HIP_TRY(hipMemcpy(out, d_buf, bytes, hipMemcpyDeviceToHost));
  return NRPHY_OK;
}
