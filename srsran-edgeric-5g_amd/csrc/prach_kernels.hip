// PRACH generator and detector kernels for gfx950 (MI355X).
//
// Replaces prach_generator_impl::generate (R/lib/phy/upper/channel_processors/prach_generator_impl.cpp:97-287) and
// prach_detector_generic_impl::detect (prach_detector_generic_impl.cpp:89-359, symbols combined).  Three launches per run:
//   1. prach_rssi_kernel: one wavefront per occasion; the RSSI and the constant fields of the result header.
//   2. prach_detect_kernel<N, L, WAVES>: one workgroup of WAVES wavefronts per (occasion, root sequence).  The root's
//      frequency-domain sequence is built once into LDS.  Per pass each wavefront takes one receive port: the symbols are
//      summed, multiplied by the conjugate root and placed on the bins of the N-point inverse transform while they are loaded
//      into the first butterfly's registers; the transform runs in LDS (the Stockham stages of fft_device.h, 64 threads each)
//      and its sink leaves |.|^2 / (N L^2) in the transform's own buffer.  The cyclic shift windows are then shared out among
//      groups of lanes (as many lanes as a window is wide, rounded up to a power of two): a group sums its window's reference
//      energy and accumulates numerator and denominator in LDS, taking the pass's ports in port order.  After the last port
//      the groups form the metric, its maximum and the decision, and write every preamble slot of the sequence exactly once.
//   3. prach_finish_kernel: one wavefront per occasion; the number of detections and their mask (a ballot, no atomics).
// Every sum has a fixed order, so two runs give identical bytes.
#include "exact_device.h"
#include "fft_device.h"

namespace nrphy {

constexpr double PRACH_T_C = 1.0 / (480000.0 * 4096.0);

// phy_time_unit::from_seconds(...).to_seconds(): rounded to the nearest multiple of T_c the way the reference does it.
__device__ __forceinline__ float round_to_tc(double seconds)
{
  const double  tc_units_dbl = seconds / PRACH_T_C;
  const int64_t tc_units     = (int64_t)(tc_units_dbl * 10.0);
  const int64_t value        = tc_units / 10 + (tc_units % 10) / 5;
  return (float)((double)value * PRACH_T_C);
}

// y[n] = table[(2 (u f n (f n + 1) + 2 C_v n) + offset) mod 4L], every product reduced mod 4L so that 32 bits suffice.
template <uint32_t L>
__device__ __forceinline__ float2 prach_sample(const float2* __restrict__ table, PrachSequence s, uint32_t n)
{
  constexpr uint32_t M  = 4 * L;
  const uint32_t     fn = ((uint32_t)s.factor * n) % M;
  const uint32_t     q  = (n * (fn + 1)) % M;
  const uint32_t     a  = (2U * (uint32_t)s.u * (uint32_t)s.factor) % M;
  const uint32_t     c  = ((4U * (uint32_t)s.shift) % M * n) % M;
  return table[(a * q + c + (uint32_t)s.offset) % M];
}

template <uint32_t L>
__global__ __launch_bounds__(64) void prach_generate_kernel(const PrachTables* __restrict__ tables, PrachSequence s,
                                                            float2* __restrict__ y)
{
  const float2* table = L == PRACH_L_LONG ? tables->cexp_long : tables->cexp_short;
  for (uint32_t n = threadIdx.x; n < L; n += 64) {
    y[n] = prach_sample<L>(table, s, n);
  }
}

__global__ __launch_bounds__(64) void prach_rssi_kernel(PrachLaunch p)
{
  const uint32_t   occ = blockIdx.x, lane = threadIdx.x;
  const PrachDesc& d   = p.desc[occ];
  const uint32_t   L   = d.is_long ? PRACH_L_LONG : PRACH_L_SHORT;
  double           acc = 0;
  for (uint32_t port = 0; port != d.nof_rx_ports; ++port) {
    for (uint32_t sym = 0; sym != d.nof_symbols; ++sym) {
      const float2* x = p.symbols + d.sym_offset + port * p.port_stride + sym * p.symbol_stride;
      for (uint32_t k = lane; k < L; k += 64) {
        const float2 v = x[k];
        acc += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
      }
    }
  }
  acc = wave_sum(acc);
  // The reference divides the mean power per symbol by (ports x symbols x L) once more; so does this.
  const float rssi = (float)(acc / (double)L / (double)(d.nof_rx_ports * d.nof_symbols * L));
  if (lane == 0) {
    p.result[occ].rssi_dB            = 10.0f * log10f(rssi);
    p.result[occ].time_resolution_s  = d.time_resolution_s;
    p.result[occ].time_advance_max_s = d.time_advance_max_s;
    p.rssi_ok[occ]                   = is_normal(rssi) ? 1U : 0U;
  }
}

__global__ __launch_bounds__(64) void prach_finish_kernel(PrachLaunch p)
{
  const uint32_t occ  = blockIdx.x, lane = threadIdx.x;
  const uint64_t mask = __ballot(p.preambles[(size_t)occ * NRPHY_PRACH_MAX_PREAMBLES + lane].detected != 0);
  if (lane == 0) {
    p.result[occ].nof_detected  = (uint32_t)__popcll(mask);
    p.result[occ].detected_mask = mask;
  }
}

// (x[0] + x[stride] + ... , symbols in order) x conj(root): one frequency-domain sample of the correlation's input.
__device__ __forceinline__ cf combined_times_conj_root(const float2* __restrict__ x, uint32_t nof_symbols, uint64_t symbol_stride, cf r)
{
  float2 sum = x[0];
  for (uint32_t sym = 1; sym != nof_symbols; ++sym) {
    const float2 t = x[sym * symbol_stride];
    sum.x += t.x;
    sum.y += t.y;
  }
  return make_cf(sum.x * r.x + sum.y * r.y, sum.y * r.x - sum.x * r.y);
}

// Transforms in flight per workgroup: one wavefront each, on consecutive receive ports (A/B builds: 1, 2 or 4).
#ifndef NRPHY_PRACH_WAVES
#define NRPHY_PRACH_WAVES 4
#endif
constexpr int PRACH_WAVES = NRPHY_PRACH_WAVES;

template <int N, uint32_t L, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void prach_detect_kernel(PrachLaunch p)
{
  static_assert(Plan<N>::T == 64, "one wavefront per transform");
  constexpr uint32_t T = 64 * WAVES;
  __shared__ cf    lds[WAVES][N + N / 16 + 16];
  __shared__ cf    root[L];
  __shared__ float num[N], den[N];
  const uint32_t   tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const uint32_t   job = (L == PRACH_L_LONG ? p.jobs_long : p.jobs_short)[blockIdx.x];
  const uint32_t   occ = job >> 8, seq = job & 255U;
  const PrachDesc& d   = p.desc[occ];
  const uint32_t   win = d.win_width, nof_shifts = d.nof_shifts;
  const uint32_t   first = seq * nof_shifts; // preamble index of window 0
  const bool       run   = p.rssi_ok[occ] != 0 && first < d.end && first + nof_shifts > d.start;
  // Lanes per window (a group never straddles a wavefront) and windows per pass.
  const uint32_t lg = d.group_log2, group = 1U << lg, s0 = tid & (group - 1), wl = tid >> lg, per_pass = T >> lg;

  if (run) {
    const float2* table = L == PRACH_L_LONG ? p.tables->cexp_long : p.tables->cexp_short;
    const float2* tw    = L == PRACH_L_LONG ? p.tables->tw_long : p.tables->tw_short;
    for (uint32_t n = tid; n < L; n += T) {
      const float2 y = prach_sample<L>(table, d.seq[seq], n);
      root[n]        = make_cf(y.x, y.y);
    }
    for (uint32_t i = tid; i < nof_shifts * win; i += T) {
      num[i] = 0.f;
      den[i] = 0.f;
    }
    const TwiddleBase<N> tb = load_twiddle_base<+1, N>(tw, lane);
    __syncthreads();
    for (uint32_t port0 = 0; port0 < d.nof_rx_ports; port0 += WAVES) {
      // Wavefront `wave` transforms port port0 + wave (zeros beyond the last port: every wavefront meets every barrier).
      const uint32_t port = port0 + wave;
      const float2*  x    = p.symbols + d.sym_offset + port * p.port_stride;
      const uint32_t nof_here = min((uint32_t)WAVES, d.nof_rx_ports - port0);
      cf a[Plan<N>::R0];
#pragma unroll
      for (int k = 0; k != Plan<N>::R0; ++k) {
        // Bin i of the transform: the last L/2 + 1 products on bins [0, L/2], the first L/2 on the top bins, zeros between.
        const uint32_t i   = first_stage_index<N>(lane, k);
        const bool     low = i <= L / 2, high = i >= N - L / 2 && i < (uint32_t)N;
        const uint32_t src = low ? i + L / 2 : i - (N - L / 2);
        cf             v   = make_cf(0.f, 0.f);
        if ((low || high) && port < d.nof_rx_ports && (N / Plan<N>::R0 >= 64 || lane < (uint32_t)(N / Plan<N>::R0))) {
          v = combined_times_conj_root(x + src, d.nof_symbols, p.symbol_stride, root[src]);
        }
        a[k] = v;
      }
      // The last stage's sink leaves |.|^2 / (N L^2) in the transform's own buffer, once every thread has read its inputs.
      float*      mine  = (float*)lds[wave];
      const float scale = d.modsq_scale;
      auto        store = [&](uint32_t q, auto base, auto, cf v) { mine[q + decltype(base)::value] = (v.x * v.x + v.y * v.y) * scale; };
      fft_from_registers<+1, N>(a, tb, lds[wave], tw, lane, store);
      // The windows, shared out among all the workgroup's groups of lanes; each takes this pass's ports in port order.
      for (uint32_t wb = 0; wb < nof_shifts; wb += per_pass) {
        const uint32_t w      = wb + wl;
        const bool     active = w < nof_shifts;
        const uint32_t ws     = active ? (N - (d.n_cs * w * N) / L) % N : 0U;
        const uint32_t i_start = (ws + N - d.win_margin) % N, len = 2 * d.win_margin + win;
        for (uint32_t pp = 0; pp != nof_here; ++pp) {
          const float* modsq = (const float*)lds[pp];
          float        ref   = 0.f;
          if (active) {
            for (uint32_t j = s0; j < len; j += group) {
              const uint32_t i = i_start + j;
              ref += modsq[i >= (uint32_t)N ? i - N : i];
            }
          }
          for (uint32_t m = 1; m < group; m <<= 1) {
            ref += __shfl_xor(ref, (int)m);
          }
          if (active) {
            for (uint32_t s = s0; s < win; s += group) {
              const float v    = modsq[ws + s] * d.win_scale;
              float       diff = ref - v;
              if (!is_normal(diff)) {
                diff = 1e-9f;
              }
              num[w * win + s] += v;
              den[w * win + s] += diff;
            }
          }
        }
      }
      __syncthreads(); // the next transforms overwrite the buffers
    }
  }

  // Every preamble slot of this sequence is written once: the metric's window, its maximum and the decision where the preamble
  // is monitored and the occasion has a normal RSSI, zeros otherwise.
  for (uint32_t wb = 0; wb < nof_shifts; wb += per_pass) {
    const uint32_t w = wb + wl, pre = first + w;
    const bool     slot = w < nof_shifts && pre < NRPHY_PRACH_MAX_PREAMBLES;
    const bool     live = slot && run && pre >= d.start && pre < d.end;
    float          best = -INFINITY;
    uint32_t       best_i = 0xFFFFFFFFU;
    float*         row = (p.metric != nullptr && slot) ? p.metric + ((size_t)occ * NRPHY_PRACH_MAX_PREAMBLES + pre) * p.metric_stride : nullptr;
    for (uint32_t s = s0; s < p.metric_stride; s += group) {
      float m = 0.f;
      if (live && s < win) {
        m = num[w * win + s] / fabsf(den[w * win + s]);
        if (m > best) {
          best   = m;
          best_i = s;
        }
      }
      if (row != nullptr) {
        row[s] = m;
      }
    }
    for (uint32_t m = 1; m < group; m <<= 1) { // the largest value; on a tie the lowest index
      const float    ov = __shfl_xor(best, (int)m);
      const uint32_t oi = (uint32_t)__shfl_xor((int)best_i, (int)m);
      if (ov > best || (ov == best && oi < best_i)) {
        best   = ov;
        best_i = oi;
      }
    }
    if (slot && s0 == 0) {
      nrphy_prach_preamble_t out = {0, 0, 0.f, 0.f, 0.f};
      if (live && best_i < win) {
        out.detected         = (best > d.threshold && best_i < d.delay_end) ? 1U : 0U;
        out.delay_samples    = best_i;
        out.time_advance_s   = round_to_tc((double)best_i / d.sample_rate_hz);
        out.peak             = best;
        out.detection_metric = best / d.threshold;
      }
      p.preambles[(size_t)occ * NRPHY_PRACH_MAX_PREAMBLES + pre] = out;
    }
  }
}

hipError_t launch_prach_detect(const PrachLaunch& p, hipStream_t stream)
{
  hipLaunchKernelGGL(prach_rssi_kernel, dim3(p.n), dim3(64), 0, stream, p);
  if (p.n_jobs_long != 0) {
    hipLaunchKernelGGL((prach_detect_kernel<(int)PRACH_N_LONG, PRACH_L_LONG, PRACH_WAVES>), dim3(p.n_jobs_long), dim3(64 * PRACH_WAVES), 0, stream, p);
  }
  if (p.n_jobs_short != 0) {
    hipLaunchKernelGGL((prach_detect_kernel<(int)PRACH_N_SHORT, PRACH_L_SHORT, PRACH_WAVES>), dim3(p.n_jobs_short), dim3(64 * PRACH_WAVES), 0, stream,
                       p);
  }
  hipLaunchKernelGGL(prach_finish_kernel, dim3(p.n), dim3(64), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_prach_generate(const PrachTables* tables, PrachSequence seq, uint32_t is_long, float2* d_y, hipStream_t stream)
{
  if (is_long) {
    hipLaunchKernelGGL(prach_generate_kernel<PRACH_L_LONG>, dim3(1), dim3(64), 0, stream, tables, seq, d_y);
  } else {
    hipLaunchKernelGGL(prach_generate_kernel<PRACH_L_SHORT>, dim3(1), dim3(64), 0, stream, tables, seq, d_y);
  }
  return hipGetLastError();
}

} // namespace nrphy
