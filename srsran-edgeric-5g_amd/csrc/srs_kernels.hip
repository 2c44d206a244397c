// SRS channel estimator for gfx950: grid to the wideband channel matrix and the time alignment of a sounding reference signal.
//
// Replaces srs_estimator_generic_impl::estimate (R/lib/phy/upper/signal_processors/srs/srs_estimator_generic_impl.cpp:62-193) with
// the sequences of low_papr_sequence_generator_impl::generate and the search of time_alignment_estimator_dft_impl::estimate
// (time_alignment_estimator_dft_impl.cpp:79-105).
//
// Two launches of one 256-thread workgroup per (SRS, receive port, antenna port): the common time alignment averages over all
// paths before any path can be compensated, and a workgroup per path keeps a 4 x 4 SRS at one transform's latency, not sixteen.
//  srs_ta_kernel    thread t owns the transform inputs x[t + 256 k], k < 16.  Input i is non-zero only where i mod comb = 0 and
//                   i / comb < M; the thread builds those mean LS estimates itself (srs_mean_lse: sequence value, grid words of
//                   every symbol), nothing goes through LDS.  The 4096-point inverse transform (fft_device.h) ends in a sink that
//                   keeps |X|^2 of the bins [0, W) and [4096 - W, 4096) only -- at most one of each per thread --, a workgroup
//                   reduction takes the maximum of each side, the lower bin among equals, and the delay wins ties.  Writes
//                   ta_bins[rx][tx]; workgroups beyond the configured ports write 0.
//  srs_coef_kernel  every workgroup recomputes the average of bins / (4096 scs) in double from the sixteen integers, antenna port
//                   outer and receive port inner, then its path's mean LS estimates again (the grid words are few; this is what
//                   avoids scratch), times the 1024-point unit circle at an index evaluated in single precision operation by
//                   operation, and their mean.  Writes h[rx][tx] (0 beyond the configured ports); the workgroup of path (0, 0)
//                   writes time_alignment_s and the padding.
// No atomics, no scratch; contraction is off, fused multiply-adds only where written.
#include "bits_device.h"
#include "exact_device.h"
#include "fft_device.h"
#include "low_papr_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t SRS_THREADS = Plan<SRS_DFT_SIZE>::T; // 256
constexpr uint32_t SRS_WAVES   = SRS_THREADS / WAVE;
static_assert(SRS_MAX_SEQ * 2 <= SRS_DFT_SIZE, "the sequence on its comb fits the transform");

typedef const NRPHY_CONSTANT SrsDesc& SrsDescRef;

// low_papr_sequence_generator_impl::generate(u, 0, n_cs, n_cs_max)[n] for antenna port `port`.
__device__ __forceinline__ float2 srs_sequence(SrsDescRef d, const float2* __restrict__ cs_table, uint32_t port, uint32_t n)
{
  float2 r; // the element's entry of its unit circle is low_papr_device.h's
  if (d.M < 36u) {
    r = unit_circle(low_papr_table_index(d.phi[n]), LOW_PAPR_TABLE_CIRCLE);
  } else {
    r = unit_circle(low_papr_zc_index(d.q, d.n_zc, n), 2u * d.n_zc);
  }
  const uint32_t step = d.cs_step[port];
  if (step != 0u) {
    r = exact::cmul(r, cs_table[(n * step) % SRS_CS_SIZE]);
  }
  return r;
}

// Element n of the path's mean LS estimate: y conj(r) on the first symbol, the further symbols added in order, scaled by
// float(1.0 / nof_symbols) when there is more than one.  `row` is the first symbol's row of the receive port.
__device__ __forceinline__ float2 srs_mean_lse(SrsDescRef d, const SrsLaunch& p, const uint32_t* __restrict__ row, uint32_t port, uint32_t n)
{
  const float2   r = srs_sequence(d, p.cs_table, port, n);
  const uint32_t k = d.k0[port] + d.comb * n;
  float2         acc = make_float2(0.f, 0.f);
  for (uint32_t l = 0; l != d.nof_symbols; ++l) {
    const float2 y = cbf16_to_float2(row[(size_t)l * p.grid_nof_subc + k]);
    const float2 e = exact::mul_conj(y, r);
    acc            = l == 0u ? e : make_float2(__fadd_rn(acc.x, e.x), __fadd_rn(acc.y, e.y));
  }
  if (d.nof_symbols > 1u) {
    acc = make_float2(__fmul_rn(acc.x, d.symbol_scale), __fmul_rn(acc.y, d.symbol_scale));
  }
  return acc;
}

__device__ __forceinline__ const uint32_t* srs_row(SrsDescRef d, const SrsLaunch& p, uint32_t rx)
{
  return p.grid + (((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[rx]) * NRPHY_NSYMB + d.first_symbol) * p.grid_nof_subc;
}

__global__ __launch_bounds__(SRS_THREADS) void srs_ta_kernel(SrsLaunch p)
{
  __shared__ cf       lds[SRS_DFT_SIZE + SRS_DFT_SIZE / 16 + 16];
  __shared__ float    red_m[2][SRS_WAVES];
  __shared__ uint32_t red_i[2][SRS_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t rx = blockIdx.x / NRPHY_MAX_PORTS, tx = blockIdx.x % NRPHY_MAX_PORTS, is = blockIdx.y;
  SrsDescRef     d  = *to_constant(p.desc + is);
  int32_t*       out = &p.result[is].ta_bins[rx][tx];
  if (rx >= d.nof_rx_ports || tx >= d.nof_tx_ports) { // workgroup-uniform
    if (tid == 0) {
      *out = 0;
    }
    return;
  }
  const uint32_t* row = srs_row(d, p, rx);
  const uint32_t  comb = d.comb, M = d.M, W = d.window;
  cf              a[16];
#pragma unroll
  for (int k = 0; k != 16; ++k) {
    const uint32_t i = first_stage_index<SRS_DFT_SIZE>(tid, k), n = i / comb;
    float2         v = make_float2(0.f, 0.f);
    if (i % comb == 0u && n < M) {
      v = srs_mean_lse(d, p, row, tx, n);
    }
    a[k] = make_cf(v.x, v.y);
  }
  const TwiddleBase<SRS_DFT_SIZE> tb = load_twiddle_base<+1, SRS_DFT_SIZE>(p.twiddle, tid);
  // Output q + 256 j of the last stage: the delays [0, W) are outputs j = 0 of threads q < W, the advances [4096 - W, 4096) are
  // outputs j = 15 of threads q >= 256 - W (W <= 256).
  float    best_d = -1.f, best_a = -1.f;
  uint32_t id = 0, ia = 0;
  auto     sink = [&](uint32_t q, auto base, auto, cf v) {
    constexpr uint32_t B = decltype(base)::value;
    if constexpr (B == 0u || B == SRS_DFT_SIZE - SRS_THREADS) {
      const float m = exact::norm(make_float2(v.x, v.y));
      if (B == 0u) {
        if (q < W) {
          take_max(best_d, id, m, q);
        }
      } else if (q + W >= SRS_THREADS) {
        take_max(best_a, ia, m, q + W - SRS_THREADS); // index within the last W bins
      }
    }
  };
  fft_from_registers<+1, SRS_DFT_SIZE>(a, tb, lds, p.twiddle, tid, sink);
  wave_take_max(best_d, id, best_a, ia);
  if (lane == 0) {
    red_m[0][wave] = best_d;
    red_i[0][wave] = id;
    red_m[1][wave] = best_a;
    red_i[1][wave] = ia;
  }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w != SRS_WAVES; ++w) {
      take_max(best_d, id, red_m[0][w], red_i[0][w]);
      take_max(best_a, ia, red_m[1][w], red_i[1][w]);
    }
    *out = ta_signed_bin(best_d, id, best_a, ia, W); // -(W - ia)
  }
}

__global__ __launch_bounds__(SRS_THREADS) void srs_coef_kernel(SrsLaunch p)
{
  __shared__ float2 red[SRS_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t rx = blockIdx.x / NRPHY_MAX_PORTS, tx = blockIdx.x % NRPHY_MAX_PORTS, is = blockIdx.y;
  SrsDescRef          d = *to_constant(p.desc + is);
  nrphy_srs_result_t& res = p.result[is];
  // The common time alignment: to_seconds of every path, added antenna port outer and receive port inner, over the path count.
  const double rate = (double)(SRS_DFT_SIZE * d.scs_hz);
  double       ta   = 0.0;
  for (uint32_t t = 0; t != d.nof_tx_ports; ++t) {
    for (uint32_t r = 0; r != d.nof_rx_ports; ++r) {
      ta += (double)res.ta_bins[r][t] / rate;
    }
  }
  ta /= (double)(d.nof_tx_ports * d.nof_rx_ports);
  if (blockIdx.x == 0 && tid == 0) {
    res.time_alignment_s = ta;
    res.reserved_[0]     = 0;
    res.reserved_[1]     = 0;
  }
  if (rx >= d.nof_rx_ports || tx >= d.nof_tx_ports) { // workgroup-uniform
    if (tid == 0) {
      res.h_re[rx][tx] = 0.f;
      res.h_im[rx][tx] = 0.f;
    }
    return;
  }
  // TWOPI * ta * scs_to_khz(scs) * 1000 * comb_size, left to right in double, then the offset in float.
  const float fcomb = (float)d.comb;
  const float ps    = (float)((((double)TWOPI_F * ta) * (double)(d.scs_hz / 1000u)) * 1000.0 * (double)d.comb);
  const float off   = __fdiv_rn(__fmul_rn(ps, (float)(d.k0[tx] % d.comb)), fcomb);
  const uint32_t* row = srs_row(d, p, rx);
  float2 sum = make_float2(0.f, 0.f);
  for (uint32_t n = tid; n < d.M; n += SRS_THREADS) {
    const float2 e = srs_mean_lse(d, p, row, tx, n);
    // round(1024 * (n * ps + offset) / TWOPI): every step in single precision, half away from zero, negative values wrapped.
    const float  x   = __fdiv_rn(__fmul_rn((float)SRS_CEXP_SIZE, __fadd_rn(__fmul_rn((float)n, ps), off)), TWOPI_F);
    const int    idx = (int)roundf(x);
    const float2 c   = exact::cmul(e, p.cexp_table[(uint32_t)idx % SRS_CEXP_SIZE]);
    sum              = make_float2(__fadd_rn(sum.x, c.x), __fadd_rn(sum.y, c.y));
  }
#pragma unroll
  for (int o = WAVE / 2; o != 0; o >>= 1) {
    sum = make_float2(__fadd_rn(sum.x, __shfl_xor(sum.x, o)), __fadd_rn(sum.y, __shfl_xor(sum.y, o)));
  }
  if (lane == 0) {
    red[wave] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w != SRS_WAVES; ++w) {
      sum = make_float2(__fadd_rn(sum.x, red[w].x), __fadd_rn(sum.y, red[w].y));
    }
    const float fm   = (float)d.M;
    res.h_re[rx][tx] = __fdiv_rn(sum.x, fm);
    res.h_im[rx][tx] = __fdiv_rn(sum.y, fm);
  }
}

__global__ __launch_bounds__(SRS_THREADS) void srs_sequence_kernel(const SrsDesc* desc, const float2* cs_table, uint32_t port, uint32_t M, float2* out)
{
  SrsDescRef     d = *to_constant(desc);
  const uint32_t n = blockIdx.x * SRS_THREADS + threadIdx.x;
  if (n < M) {
    out[n] = srs_sequence(d, cs_table, port, n);
  }
}

} // namespace

hipError_t launch_srs(const SrsLaunch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(srs_ta_kernel, dim3(SRS_PATHS, p.n), dim3(SRS_THREADS), 0, stream, p);
  hipLaunchKernelGGL(srs_coef_kernel, dim3(SRS_PATHS, p.n), dim3(SRS_THREADS), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_srs_sequence(const SrsDesc* desc, const float2* cs_table, uint32_t port, uint32_t M, float2* out, hipStream_t stream)
{
  hipLaunchKernelGGL(srs_sequence_kernel, dim3((M + SRS_THREADS - 1) / SRS_THREADS), dim3(SRS_THREADS), 0, stream, desc, cs_table, port, M, out);
  return hipGetLastError();
}

} // namespace nrphy
