// OFDM PRACH demodulator kernel for gfx950 (MI355X).
//
// Replaces ofdm_prach_demodulator_impl::demodulate (R/lib/phy/lower/modulation/ofdm_prach_demodulator_impl.cpp:158-201): the
// direct, unnormalised transform of every PRACH symbol and the copy of the L_RA bins of every frequency-domain occasion into the
// prach_buffer.  One workgroup per (item, port, time-domain occasion, symbol); the plan has done the window and bin arithmetic.
//
// dft_size <= 6144: one Stockham transform in LDS (fft_device.h).  Its sink looks at the bin it is handed, and stores it at its
// place in the buffer when it belongs to an occasion: nothing else of the spectrum is written anywhere.
//
// dft_size = N1 x N2 (N1 in {3, 6, 12}, N2 in {3072, 4096}): the INPUT is decimated, Y_r = DFT_N2(x[N1 m + r]), and
//   X[k] = sum_{r < N1} W_N^(r k) Y_r[k mod N2],
// so the workgroup runs N1 LDS transforms one after the other and its sink adds term r to the wanted bins only: bin k of pass r
// is always handed to the same thread, which therefore keeps the running sum in the output element itself (pass 0 stores, the
// later passes read, add and store; fixed order, no atomics, no scratch copy of the batch and no second launch).  The loads of
// pass r are N1 elements apart: every cache line of the symbol is touched N1 times, out of L2 after the first.
//
// The wanted bins are nof_fd runs of L_RA, `spacing` bins apart, from first_bin on modulo dft_size.  With rel = (bin - first_bin)
// mod dft_size a bin is wanted iff rel < span and rel mod spacing < L_RA.  A sink holds bin j of the N2-point transform, that is
// the bins j, j + N2, ... of X: rel runs over (j - first_bin) mod N2 + t N2 below span.
//
// The samples come as complex float (IQ_CI16 = false) or as the radio's complex int16 (true), as in ofdm_demod_kernel: two int16
// per sample at the same sample index, each widened as srsvec::convert does (R/lib/srsvec/conversion.cpp:67-129), float(x) * gain
// with gain = 1 / scale rounded once on the host, the product a value of its own before the first butterfly.  A lane takes the
// registers of its first stage straight from memory in both formats, so it loads one 4-byte sample where the float instance
// loads 8 bytes: consecutive lanes read consecutive samples (256 contiguous bytes per wave and load in the single transform, one
// sample in n1 on the decimated path, where the other n1 - 1 passes find the lines in L2 as before).  A wider load per lane would
// want the lane to own neighbouring samples, which the first stage's x[tid + k N / R0] does not give it without a pass through
// LDS.  Everything behind the load is the same code for both formats.
#include "fft_device.h"

namespace nrphy {

template <int N, bool IQ_CI16>
__global__ __launch_bounds__(Plan<N>::T) void prach_demod_kernel(PrachDemodLaunch p)
{
  __shared__ cf       lds[N + N / 16 + 16];
  const uint32_t      tid = threadIdx.x;
  const PrachDemodJob job = p.jobs[blockIdx.x];
  const PrachDemodDesc& d = p.desc[job.desc];
  const uint32_t      n1 = d.n1, n_total = d.n_total, seq_len = d.seq_len, spacing = d.spacing, span = d.span;
  const uint32_t      first_bin = d.first_bin, first_bin_lds = d.first_bin_lds;
  const uint64_t      fd_stride = d.fd_stride;
  const float2* __restrict__ tw_total = d.tw_total;
  const float2* __restrict__ in       = static_cast<const float2*>(p.samples) + job.in_offset;   // IQ_CI16 = false
  const uint32_t* __restrict__ in16   = static_cast<const uint32_t*>(p.samples) + job.in_offset; // IQ_CI16 = true
  const float         iq_gain = p.iq_gain;
  float2*             out = p.symbols + job.out_offset;
  const TwiddleBase<N> tb = load_twiddle_base<-1, N>(p.tw_lds, tid);
  for (uint32_t r = 0; r != n1; ++r) {
    cf a[Plan<N>::R0];
#pragma unroll
    for (int k = 0; k != Plan<N>::R0; ++k) {
      const uint32_t i = first_stage_index<N>(tid, k);
      if constexpr (IQ_CI16) {
        const uint32_t raw = (i < N) ? in16[(size_t)i * n1 + r] : 0u;
        cf v = make_cf(__fmul_rn((float)(int16_t)(raw & 0xFFFFu), iq_gain), __fmul_rn((float)(int16_t)(raw >> 16), iq_gain));
        asm("" : "+v"(v));
        a[k] = v;
      } else {
        const float2 v = (i < N) ? in[(size_t)i * n1 + r] : make_float2(0.f, 0.f);
        a[k]           = make_cf(v.x, v.y);
      }
    }
    auto store = [&](uint32_t q, auto base, auto, cf v) {
      const uint32_t j = q + decltype(base)::value;
      for (uint32_t rel = j >= first_bin_lds ? j - first_bin_lds : j + N - first_bin_lds; rel < span; rel += N) {
        const uint32_t fd = rel / spacing, k = rel - fd * spacing;
        if (k < seq_len) {
          float2* dst = out + fd * fd_stride + k;
          cf      x   = v;
          if (r != 0) { // term r of the bin: W_N^(r bin), the table conjugated for the direct transform
            const uint32_t bin  = first_bin + rel >= n_total ? first_bin + rel - n_total : first_bin + rel;
            const float2   w    = tw_total[(r * bin) % n_total];
            const float2   prev = *dst;
            x                   = cadd(make_cf(prev.x, prev.y), cmul(v, make_cf(w.x, -w.y)));
          }
          *dst = make_float2(x.x, x.y);
        }
      }
    };
    fft_from_registers<-1, N>(a, tb, lds, p.tw_lds, tid, store);
  }
}

template <int N>
static hipError_t launch_n(const PrachDemodLaunch& p, hipStream_t stream)
{
  if (p.ci16) {
    hipLaunchKernelGGL((prach_demod_kernel<N, true>), dim3(p.n_jobs), dim3(Plan<N>::T), 0, stream, p);
  } else {
    hipLaunchKernelGGL((prach_demod_kernel<N, false>), dim3(p.n_jobs), dim3(Plan<N>::T), 0, stream, p);
  }
  return hipGetLastError();
}

// lds_size: the size one workgroup transforms in LDS (dft_split's n2); 128 is below every grid a sequence fits.
hipError_t launch_prach_demod(uint32_t lds_size, const PrachDemodLaunch& p, hipStream_t stream)
{
  if (p.n_jobs == 0) {
    return hipSuccess;
  }
  switch (lds_size) {
    case 6144:
      return launch_n<6144>(p, stream);
    case 4608:
      return launch_n<4608>(p, stream);
    case 4096:
      return launch_n<4096>(p, stream);
    case 3072:
      return launch_n<3072>(p, stream);
    case 2048:
      return launch_n<2048>(p, stream);
    case 1536:
      return launch_n<1536>(p, stream);
    case 1024:
      return launch_n<1024>(p, stream);
    case 768:
      return launch_n<768>(p, stream);
    case 512:
      return launch_n<512>(p, stream);
    case 384:
      return launch_n<384>(p, stream);
    case 256:
      return launch_n<256>(p, stream);
    default:
      return hipErrorInvalidValue;
  }
}

} // namespace nrphy
