// Soft demodulator ("demodulation mapper") for gfx950.
//
// Replaces demodulation_mapper::demodulate_soft (R/include/srsran/phy/upper/channel_modulation/demodulation_mapper.h;
// R/lib/phy/upper/channel_modulation/demodulation_mapper_impl.cpp:33-106 and demodulation_mapper_{qpsk,qam16,qam64,qam256}.cpp).
// The reference's soft bits depend on where a symbol lies in the span handed over: the leading floor(n / B) * B symbols go
// through its AVX2 code (B = 16 QPSK, 8 16-QAM, 16 64-QAM, 4 256-QAM), the rest through its generic code, and the two round
// differently (mi355_nrphy.h, nrphy_demodulate_soft).  A thread takes two neighbouring symbols of one span and picks the
// arithmetic by their index, so every soft bit equals the reference's at the same position.
//
// HBM-bound elementwise work: 12 bytes in (symbol + noise variance) and Qm bytes out per symbol; tables (1 KB) in LDS.
#include "demod_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

template <uint32_t MOD>
__global__ __launch_bounds__(256) void demodulate_soft_kernel(DemodLaunch p, const float2* __restrict__ d_symbols,
                                                              const float* __restrict__ d_noise, int8_t* __restrict__ d_llr)
{
  __shared__ Tables t;
  if constexpr (MOD >= NRPHY_MOD_QAM64) {
    for (uint32_t k = threadIdx.x; k < DEMOD_MAX_PAIRS * 16u; k += blockDim.x) {
      t.line[k / 16u][k % 16u] = make_float2(p.slope[k / 16u][k % 16u], p.intercept[k / 16u][k % 16u]);
    }
    __syncthreads();
  }
  constexpr uint32_t qm    = MOD == NRPHY_MOD_PI2_BPSK ? 1u : MOD;
  const uint32_t     span  = blockIdx.y;
  const uint32_t     first = 2u * (blockIdx.x * blockDim.x + threadIdx.x); // the thread's first symbol
  if (first >= p.span_len) {
    return;
  }
  const uint32_t count = first + 1u < p.span_len ? 2u : 1u;
  const size_t   base  = (size_t)span * p.span_len + first;
  LlrBytes       out;
  if (count == 2u && first + 2u <= p.nof_vector) {
    // two symbols of the vector part: one 16-byte and one 8-byte load where the addresses allow
    float2 z0, z1;
    float  n0, n1;
    if (((reinterpret_cast<uintptr_t>(d_symbols + base) & 15u) | (reinterpret_cast<uintptr_t>(d_noise + base) & 7u)) == 0) {
      const float4 zz = *reinterpret_cast<const float4*>(d_symbols + base);
      const float2 nn = *reinterpret_cast<const float2*>(d_noise + base);
      z0 = make_float2(zz.x, zz.y), z1 = make_float2(zz.z, zz.w), n0 = nn.x, n1 = nn.y;
    } else {
      z0 = d_symbols[base], z1 = d_symbols[base + 1], n0 = d_noise[base], n1 = d_noise[base + 1];
    }
    demodulate_symbol<MOD, true>(p, t, first, z0.x, z0.y, n0, out, 0);
    demodulate_symbol<MOD, true>(p, t, first + 1u, z1.x, z1.y, n1, out, qm);
  } else {
#pragma unroll
    for (uint32_t s = 0; s != 2; ++s) {
      if (s < count) {
        const float2 z = d_symbols[base + s];
        if (first + s < p.nof_vector) {
          demodulate_symbol<MOD, true>(p, t, first + s, z.x, z.y, d_noise[base + s], out, s * qm);
        } else {
          demodulate_symbol<MOD, false>(p, t, first + s, z.x, z.y, d_noise[base + s], out, s * qm);
        }
      }
    }
  }
  int8_t*        dst    = d_llr + base * qm;
  const uint32_t nbytes = count * qm;
  if (nbytes == 16u && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    *reinterpret_cast<uint4*>(dst) = make_uint4(out.w[0], out.w[1], out.w[2], out.w[3]);
  } else if ((nbytes & 3u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
#pragma unroll
    for (uint32_t k = 0; k != 4; ++k) {
      if (4u * k < nbytes) {
        reinterpret_cast<uint32_t*>(dst)[k] = out.w[k];
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k != 16; ++k) {
      if (k < nbytes) {
        dst[k] = (int8_t)out.get(k);
      }
    }
  }
}

} // namespace

hipError_t launch_demodulate_soft(const DemodLaunch& p, uint32_t nof_spans, const float* d_symbols, const float* d_noise,
                                  int8_t* d_llr, hipStream_t stream)
{
  const uint32_t pairs  = (p.span_len + 1u) / 2u;
  const dim3     grid((pairs + 255u) / 256u, nof_spans), block(256);
  const float2*  sym = reinterpret_cast<const float2*>(d_symbols);
  switch (p.modulation) {
    case NRPHY_MOD_PI2_BPSK:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_PI2_BPSK>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    case NRPHY_MOD_BPSK:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_BPSK>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    case NRPHY_MOD_QPSK:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_QPSK>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    case NRPHY_MOD_QAM16:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_QAM16>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    case NRPHY_MOD_QAM64:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_QAM64>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    case NRPHY_MOD_QAM256:
      hipLaunchKernelGGL(demodulate_soft_kernel<NRPHY_MOD_QAM256>, grid, block, 0, stream, p, sym, d_noise, d_llr);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

} // namespace nrphy
