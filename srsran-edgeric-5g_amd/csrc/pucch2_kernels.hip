// PUCCH format 2 receiver for gfx950: grid to descrambled soft bits, channel state information and (optionally) the estimate.
//
// Replaces, of pucch_processor_impl::process(grid, format2_configuration)
// (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:131-215), dmrs_pucch_processor_format2_impl::estimate on
// port_channel_estimator_average_impl::compute (filter smoothing, CFO compensation on), get_channel_state_information and
// pucch_demodulator_impl::demodulate (pucch_demodulator_impl.cpp:31-87).  The UCI decoder kernel (uci_kernels.hip) follows on
// the same stream and reads the soft bits in place.
//
// One 256-thread workgroup per PUCCH: at most 4 ports x 2 symbols x 16 PRB.
//  Prologue  every wave: the twiddle table into LDS; wave p: the allocation's rows of receive port p into LDS, three 16-byte
//            words per PRB and symbol (every grid word is read once, the pilots and the data come from LDS); waves 0 and 1: the
//            DM-RS Gold words of the two symbols; wave 2: the scrambling words.
//  Estimate  wave p estimates receive port p with no workgroup barrier: a lane owns one pilot (at most 64 = 16 PRB x 4), its LS
//            products live in registers; sums are wave sums in double, folded in a fixed order; a symbol's CFO phasor is evaluated
//            once and serves derotation (conjugated), noise and the estimate's rotation; the virtual pilots are fitted by lanes 0
//            and 1 (one side each) and evaluated one per lane, and go with the FIR through the wave's LDS; the time alignment is the
//            direct partial inverse DFT over the 288 searched bins (fused multiply-adds that feed a comparison and nothing else),
//            the twiddle index reduced mod 4096 in integers, and its maximum a wave reduction that prefers the lower bin; the
//            interpolator's running sum is serial (lane 0 the real part, lane 1 the imaginary part), as the reference's is; the
//            cbf16 row of every symbol replaces the interpolated row in LDS.
//  Data      after one barrier thread t takes data RE t (at most 256 = 16 PRB x 8 x 2): equalize_re over the ports with exactly the
//            cbf16 words and noise variances written out, the QPSK demapper at position t of the span, the descrambling signs;
//            the soft bits leave through LDS as 16-byte stores.  One thread of the last wave merges the ports' measurements meanwhile.
// atan2, hypot, cos, sin and log10 are evaluated in double and rounded once.  Contraction is off.
#include "bits_device.h"
#include "chest_device.h"
#include "demod_device.h"
#include "equalize_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t PF2_THREADS    = 256;
constexpr uint32_t PF2_MAX_PILOTS = PF2_MAX_PRB * PF2_PILOTS_PER_PRB; // 64: one per lane
constexpr uint32_t PF2_MAX_SUBC   = PF2_MAX_PRB * NRPHY_NRE;          // 192
constexpr uint32_t PF2_MAX_DATA   = PF2_MAX_PRB * PF2_DATA_PER_PRB * PF2_MAX_SYMBOLS; // 256: one per thread
constexpr uint32_t PF2_V_MARGIN   = 6;                                // room for the virtual pilots at each end (at most 5)
constexpr uint32_t PF2_SEQ_WORDS  = (8 * NRPHY_MAX_RB + 31) / 32 + 1; // DM-RS Gold words from c(0): 8 bits per PRB
static_assert(PF2_SEQ_WORDS >= 2 * PF2_MAX_DATA / 32, "the scrambling words share the arrays of the DM-RS words");

struct Pf2Port {                                       // private to the wave that estimates the port
  __attribute__((aligned(16))) uint32_t rx[PF2_MAX_SYMBOLS][PF2_MAX_SUBC]; // the allocation's grid words, 16 bytes at a time
  float2   a[PF2_MAX_PILOTS + 2 * PF2_V_MARGIN];       // enlarged LS
  float2   b[PF2_MAX_PILOTS];                          // filtered pilots
  union {                                              // (a lane turns out[0][k], out[1][k] into est[0][k], est[1][k] in place)
    float    out[2][PF2_MAX_SUBC];                     // interpolated response, one plane per component
    uint32_t est[PF2_MAX_SYMBOLS][PF2_MAX_SUBC];       // the estimate as written out
  } u;
  float    jump[2][PF2_MAX_PILOTS];                    // the interpolator's steps
  float    vp_abs[2][PF2_V_MARGIN], vp_arg[2][PF2_V_MARGIN];
  VirtualPilotFit vp_fit[2];
  nrphy_pusch_chest_meas_t meas;
};

struct Pf2Shared {
  Pf2Port  port[NRPHY_MAX_PORTS];
  __attribute__((aligned(16))) float2 tw[PF2_TW_WORDS];
  uint32_t seq[3][PF2_SEQ_WORDS];                      // DM-RS words of the two symbols, scrambling words
  uint32_t gold_scratch[3][PF2_SEQ_WORDS];
  __attribute__((aligned(16))) uint8_t stage[2 * PF2_MAX_DATA];
};

// e^{j 2 pi i / 4096} from the first quadrant's table.
__device__ __forceinline__ float2 twiddle4096(const float2* tw, uint32_t i)
{
  const float2   w = tw[i & 1023u];
  const uint32_t q = (i >> 10) & 3u;
  return q == 0 ? w : q == 1 ? make_float2(-w.y, w.x) : q == 2 ? make_float2(-w.x, -w.y) : make_float2(w.y, -w.x);
}

// The plan's descriptor through the constant address space: it never changes while the kernel runs, and saying so lets its
// fields come by scalar loads that need not be repeated behind the kernel's own stores.
typedef const NRPHY_CONSTANT Pf2Desc& Pf2DescRef;

// port_channel_estimator_average_impl::compute for one receive port, by one wave.
__device__ void pf2_estimate_port(const Pf2Launch& p, Pf2DescRef d, uint32_t ip, uint32_t port, Pf2Shared& s, uint32_t lane)
{
  Pf2Port&       w  = s.port[port];
  const uint32_t N = PF2_PILOTS_PER_PRB * d.nprb, ns = d.nof_symbols, nsubc = NRPHY_NRE * d.nprb;
  const bool     mine = lane < N;
  const uint32_t k_pilot = 3u * lane + 1u; // subcarrier of the lane's pilot within the allocation: 12 (q / 4) + 3 (q % 4) + 1

  // ---- LS products, EPRE, CFO (preprocess_pilots_and_cfo) -------------------------------------------------------------------
  float2 y[PF2_MAX_SYMBOLS] = {}, pl[PF2_MAX_SYMBOLS] = {}, ls[PF2_MAX_SYMBOLS] = {};
  double epre = 0.0;
#pragma unroll
  for (uint32_t l = 0; l != PF2_MAX_SYMBOLS; ++l) {
    if (l < ns && mine) {
      pl[l] = qpsk_pilot(s.seq[l], 8u * d.prb0 + 2u * lane);
      y[l]  = cbf16_to_float2(w.rx[l][k_pilot]);
      epre += (double)exact::norm(y[l]);
      ls[l] = exact::mul_conj(y[l], pl[l]);
    }
  }
  epre       = wave_sum(epre);
  float  cfo = 0.f;
  float2 A   = ls[0];
  float2 rot[PF2_MAX_SYMBOLS] = {make_float2(1.f, 0.f), make_float2(1.f, 0.f)};
  if (ns >= 2u) { // wave-uniform
    // dot_prod(LS1, LS0) = sum LS1 conj(LS0)
    const float2 dot   = exact::mul_conj(ls[1], ls[0]);
    const double dr = wave_sum((double)dot.x), di = wave_sum((double)dot.y);
    const float  phase = (float)atan2((double)(float)di, (double)(float)dr);
    cfo                = __fdiv_rn(__fdiv_rn(phase, TWOPI_F), __fsub_rn(d.epoch[1], d.epoch[0]));
    // The phasor of a symbol, e^{j 2 pi epoch cfo}, is evaluated once: derotation uses its conjugate (the argument's sign flips
    // exactly, cos is even and sin odd), the noise and the estimate's rotation use it as it is.
    rot[0] = phasor(__fmul_rn(__fmul_rn(TWOPI_F, d.epoch[0]), cfo));
    rot[1] = phasor(__fmul_rn(__fmul_rn(TWOPI_F, d.epoch[1]), cfo));
    const float2 r0 = make_float2(rot[0].x, -rot[0].y), r1 = make_float2(rot[1].x, -rot[1].y);
    const float2 a = exact::cmul(ls[0], r0), c = exact::cmul(ls[1], r1);
    A              = make_float2(__fadd_rn(a.x, c.x), __fadd_rn(a.y, c.y));
  }
  A = make_float2(__fmul_rn(A.x, d.ls_scale), __fmul_rn(A.y, d.ls_scale)); // average; the DM-RS-to-data gain is 1
  float2* E = w.a + PF2_V_MARGIN;
  if (mine) {
    E[lane] = A;
  }
  wave_lds_fence();

  // ---- virtual pilots (add_v_pilots) and the FIR (convolution_same), the middle N outputs ---------------------------------------
  const uint32_t nv = d.nof_v;
  if (lane < 2u * nv) {
    const uint32_t side = lane / nv, i = lane % nv;
    const float2   v    = E[side == 0 ? i : N - nv + i];
    const double   re = v.x, im = v.y;
    w.vp_abs[side][i] = (float)sqrt(re * re + im * im);
    w.vp_arg[side][i] = (float)atan2(im, re);
  }
  wave_lds_fence();
  if (lane < 2u) { // the fit is serial: one lane per side
    w.vp_fit[lane] = virtual_pilot_fit(w.vp_abs[lane], w.vp_arg[lane], nv);
  }
  wave_lds_fence();
  if (lane < 2u * nv) { // the values: one lane each
    const uint32_t side = lane / nv, i = lane % nv;
    (side == 0 ? E - nv : E + N)[i] = virtual_pilot_value(w.vp_fit[side], side == 0 ? (int)i - (int)nv : (int)(i + nv));
  }
  wave_lds_fence();
  const uint32_t T = d.ntaps, mid = T / 2u;
  float2         f = make_float2(0.f, 0.f);
  if (mine) {
    const float2* x = E + lane - mid;
    for (uint32_t i = 0; i != T; ++i) {
      const float h = d.taps[T - 1u - i];
      f             = make_float2(__fadd_rn(f.x, __fmul_rn(x[i].x, h)), __fadd_rn(f.y, __fmul_rn(x[i].y, h)));
    }
    w.b[lane] = f;
  }
  const double pw   = wave_sum(mine ? (double)exact::norm(f) : 0.0);
  const float  rsrp = (float)(pw / (double)N);

  // ---- noise (estimate_noise) ---------------------------------------------------------------------------------------------------
  double ne = 0.0;
#pragma unroll
  for (uint32_t l = 0; l != PF2_MAX_SYMBOLS; ++l) {
    if (l < ns) { // wave-uniform
      float2 e = exact::cmul(make_float2(__fmul_rn(f.x, -1.0f), __fmul_rn(f.y, -1.0f)), pl[l]);
      if (ns >= 2u) {
        e = exact::cmul(e, rot[l]);
      }
      e = make_float2(__fadd_rn(e.x, y[l].x), __fadd_rn(e.y, y[l].y));
      ne += mine ? (double)exact::norm(e) : 0.0;
    }
  }
  ne = wave_sum(ne); // (its shuffles also order the writes of b)
  wave_lds_fence();

  // ---- time alignment: |IDFT_4096|^2 of the filtered pilots at their grid subcarriers, bins [0, 144) and [3952, 4096) -----------
  float    best_d = -1.f, best_a = -1.f;
  uint32_t id = 0, ia = 0;
  {
    const uint32_t k0 = NRPHY_NRE * d.prb0 + 1u; // grid subcarrier of pilot 0; pilot q sits 3 q above it
    for (uint32_t b = lane; b < CHEST_TA_BINS; b += WAVE) {
      const uint32_t n    = b < PUSCH_CHEST_TA_WINDOW ? b : 4096u - CHEST_TA_BINS + b;
      const uint32_t step = (3u * n) & 4095u;
      uint32_t       i    = (k0 * n) & 4095u;
      float2         acc  = make_float2(0.f, 0.f);
      for (uint32_t q = 0; q != N; ++q) {
        dft_accumulate(acc, w.b[q], twiddle4096(s.tw, i));
        i = (i + step) & 4095u;
      }
      const float m = exact::norm(acc);
      if (b < PUSCH_CHEST_TA_WINDOW) {
        take_max(best_d, id, m, b);
      } else {
        take_max(best_a, ia, m, b - PUSCH_CHEST_TA_WINDOW);
      }
    }
    wave_take_max(best_d, id, best_a, ia);
  }
  const int ta_bins = ta_signed_bin(best_d, id, best_a, ia, PUSCH_CHEST_TA_WINDOW);

  // ---- measurements ---------------------------------------------------------------------------------------------------------------
  const nrphy_pusch_chest_meas_t m = chest_measurements(rsrp, (float)(epre / (double)(N * ns)), (float)(ne / (double)(N * ns - 1u)), 1.0f,
                                                        ta_bins, ns >= 2u, cfo, d.scs_hz);
  if (lane == 0) {
    w.meas = m;
    if (p.meas != nullptr) {
      p.meas[(size_t)ip * NRPHY_MAX_PORTS + port] = m;
    }
  }

  // ---- linear interpolation (interpolator_linear_impl, offset 1, stride 3): the steps in parallel, the running sum serial --------
  if (lane + 1u < N) {
    const float2 f1 = w.b[lane + 1u];
    w.jump[0][lane] = __fdiv_rn(__fsub_rn(f1.x, f.x), 3.0f);
    w.jump[1][lane] = __fdiv_rn(__fsub_rn(f1.y, f.y), 3.0f);
  }
  wave_lds_fence();
  if (lane < 2u) { // lane 0: real part, lane 1: imaginary part
    const float* j   = w.jump[lane];
    float*       out = w.u.out[lane];
    float        v   = lane == 0 ? w.b[0].x : w.b[0].y;
    out[0]           = v;
    out[1]           = v;
    for (uint32_t i = 0; i + 1u < N; ++i) {
      const float h = j[i];
#pragma unroll
      for (uint32_t k = 0; k != 3; ++k) {
        v                    = __fadd_rn(v, h);
        out[3u * i + 2u + k] = v;
      }
    }
    out[nsubc - 1u] = lane == 0 ? w.b[N - 1u].x : w.b[N - 1u].y;
  }
  wave_lds_fence();

  // ---- cbf16, then per symbol the CFO phasor and cbf16 again: into LDS for the equaliser, and out -----------------------------
  for (uint32_t k = lane; k < nsubc; k += WAVE) {
    const uint32_t base = to_cbf16(w.u.out[0][k], w.u.out[1][k]);
#pragma unroll
    for (uint32_t l = 0; l != PF2_MAX_SYMBOLS; ++l) {
      if (l < ns) {
        uint32_t v = base;
        if (ns >= 2u) {
          const float2 e = exact::cmul(cbf16_to_float2(base), rot[l]);
          v              = to_cbf16(e.x, e.y);
        }
        w.u.est[l][k] = v;
        if (p.ch != nullptr) {
          p.ch[d.ce_offset + ((size_t)port * NRPHY_NSYMB + d.first_symbol + l) * p.grid_nof_subc + (size_t)NRPHY_NRE * d.prb0 + k] = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(PF2_THREADS) void pf2_kernel(Pf2Launch p)
{
  __shared__ Pf2Shared s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t ip  = blockIdx.x;
  Pf2DescRef     d   = *to_constant(p.desc + ip);
  const uint32_t P = d.nof_rx_ports, ns = d.nof_symbols, nprb = d.nprb;

  // ---- prologue ---------------------------------------------------------------------------------------------------------------
  if (wave < P) { // the port's rows: 3 nprb 16-byte words per symbol
    const uint32_t* src = p.grid + (((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[wave]) * NRPHY_NSYMB + d.first_symbol) * p.grid_nof_subc +
                          (size_t)NRPHY_NRE * d.prb0;
    for (uint32_t c = lane; c < 3u * nprb * ns; c += WAVE) {
      const uint32_t l = c / (3u * nprb), j = c - l * 3u * nprb;
      reinterpret_cast<uint4*>(s.port[wave].rx[l])[j] = reinterpret_cast<const uint4*>(src + (size_t)l * p.grid_nof_subc)[j];
    }
  }
  for (uint32_t i = tid; i < PF2_TW_WORDS / 2u; i += PF2_THREADS) {
    reinterpret_cast<uint4*>(s.tw)[i] = reinterpret_cast<const uint4*>(p.twiddle)[i];
  }
  if (wave < ns) {
    gold_sequence_wave(p.gold, p.x1_words, d.c_init_dmrs[wave], d.dmrs_words, s.seq[wave], s.gold_scratch[wave], lane);
  } else if (wave == 2u) {
    gold_sequence_wave(p.gold, p.x1_words, d.c_init_data, (16u * nprb * ns + 31u) / 32u, s.seq[2], s.gold_scratch[2], lane);
  }
  __syncthreads();

  // ---- estimation: wave p, receive port p --------------------------------------------------------------------------------------
  if (wave < P) {
    pf2_estimate_port(p, d, ip, wave, s, lane);
  } else if (p.meas != nullptr && lane == 0) {
    nrphy_pusch_chest_meas_t z = {};
    p.meas[(size_t)ip * NRPHY_MAX_PORTS + wave] = z;
  }
  __syncthreads();

  // ---- channel state information (get_channel_state_information), by one thread of the last wave --------------------------------
  if (tid == PF2_THREADS - 1u) {
    CsiMerge csi;
    for (uint32_t q = 0; q != P; ++q) {
      const nrphy_pusch_chest_meas_t& m = s.port[q].meas;
      csi.add(q, m.noise_var, m.rsrp, m.epre, m.snr, m.ta_s, m.cfo_hz);
    }
    nrphy_pf2_csi_t c  = {};
    c.sinr_dB          = csi.sinr_dB();
    c.rsrp_dB          = csi.rsrp_dB(P);
    c.epre_dB          = csi.epre_dB(P);
    c.time_alignment_s = csi.ta_s;
    c.cfo_hz           = csi.cfo_hz;
    p.csi[ip]          = c;
  }

  // ---- data: thread t, data RE t (symbol by symbol, subcarriers ascending, k mod 3 != 1) -------------------------------------------
  const uint32_t per_symbol = PF2_DATA_PER_PRB * nprb, nre = per_symbol * ns;
  if (tid < nre) {
    const uint32_t l = tid >= per_symbol ? 1u : 0u, r = tid - l * per_symbol;
    const uint32_t m = r & 7u, k = NRPHY_NRE * (r >> 3) + 3u * (m >> 1) + ((m & 1u) ? 2u : 0u);
    uint32_t       y[NRPHY_MAX_PORTS] = {}, h[2][NRPHY_MAX_PORTS] = {};
    float          nv[NRPHY_MAX_PORTS] = {};
#pragma unroll
    for (uint32_t q = 0; q != NRPHY_MAX_PORTS; ++q) {
      if (q < P) {
        y[q]    = s.port[q].rx[l][k];
        h[0][q] = s.port[q].u.est[l][k];
        nv[q]   = s.port[q].meas.noise_var;
      }
    }
    float2 x[2];
    float  v[2];
    equalize_re(NRPHY_EQ_ZF, 1u, P, y, h, nv, max_noise(nv, P), 1.0f, x, v);
    DemodLaunch dm = {};
    dm.range = p.demod_range;
    dm.scale = p.demod_scale;
    Tables   unused_tables = {}; // QPSK reads no table
    LlrBytes out;
    if (tid < d.nof_vector) {
      demodulate_symbol<NRPHY_MOD_QPSK, true>(dm, unused_tables, tid, x[0].x, x[0].y, v[0], out, 0);
    } else {
      demodulate_symbol<NRPHY_MOD_QPSK, false>(dm, unused_tables, tid, x[0].x, x[0].y, v[0], out, 0);
    }
    const uint32_t b0   = 2u * tid; // the RE's two scrambling bits: even, both in one word
    const uint32_t bits = (s.seq[2][b0 >> 5] >> (30u - (b0 & 31u))) & 3u;
    out.w[0]            = negate_bytes(out.w[0], byte_masks_msb_first(bits << 2));
    reinterpret_cast<uint16_t*>(s.stage)[tid] = (uint16_t)out.w[0];
  }
  __syncthreads();
  int8_t* dst = p.llr + d.llr_offset;
  if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) { // E is a multiple of 16
    if (tid < nre / 8u) {
      reinterpret_cast<uint4*>(dst)[tid] = reinterpret_cast<const uint4*>(s.stage)[tid];
    }
  } else if (tid < nre) {
    dst[2u * tid]      = (int8_t)s.stage[2u * tid];
    dst[2u * tid + 1u] = (int8_t)s.stage[2u * tid + 1u];
  }
}

} // namespace

hipError_t launch_pf2(const Pf2Launch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pf2_kernel, dim3(p.n), dim3(PF2_THREADS), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
