// The PUSCH DM-RS channel estimator's first kernel as a template over the source of its pilots (see pusch_chest_kernels.hip for
// the whole picture).  Each instantiation lives in a translation unit of its own -- pusch_chest_kernels.hip has the Gold one,
// pusch_chest_lowpapr_kernels.hip the low-PAPR one --, so that the Gold instantiation is compiled in a module that holds exactly
// what it held before there was a second source: in one module the second instantiation moved three of its instructions.
#pragma once

#include "bits_device.h"
#include "chest_device.h"
#include "low_papr_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t CHEST_THREADS = 256;
constexpr uint32_t MAX_PILOTS    = NRPHY_MAX_RB * 6;
constexpr uint32_t V_MARGIN      = 12;                            // MAX_V_PILOTS: room for virtual pilots at each end
constexpr uint32_t MAX_SEQ_WORDS = (NRPHY_MAX_RB * NRPHY_NRE + 31) / 32;
constexpr uint32_t TA_BINS       = CHEST_TA_BINS;

// Where the pilots come from: a compile-time parameter of pusch_chest_kernel, one instantiation each.
enum PilotSource : uint32_t { PILOT_GOLD = 0, PILOT_LOW_PAPR = 1 };

struct GoldPilots {
  uint32_t seq[NRPHY_NSYMB][MAX_SEQ_WORDS];  // Gold words c(0 ...) of every DM-RS symbol
  uint32_t scratch[4][MAX_SEQ_WORDS];
};
struct ChestShared {
  union {
    GoldPilots gold;
    uint16_t   lp_index[MAX_PILOTS];         // low-PAPR DM-RS: the pilot's entry of the unit circle, the same on every DM-RS symbol
  } pil;
  uint16_t prbs[NRPHY_MAX_RB];
  float2   a[MAX_PILOTS + 2 * V_MARGIN];     // enlarged LS; later the interpolator's half steps (two planes)
  float2   b[MAX_PILOTS];                    // LS of the second DM-RS symbol; later the filtered pilots
  union {
    float2 tw[2048];                         // e^{j 2 pi i / 2048}
    float  out[2][2 * MAX_PILOTS];           // interpolated response, one plane per component
  } u;
  float    mag[TA_BINS];
  double   red[4][2];
  float    vp_abs[2][V_MARGIN], vp_arg[2][V_MARGIN];
};

// Workgroup sum of two doubles in a fixed order; every thread gets the result.
__device__ __forceinline__ double2 block_sum2(double x, double y, ChestShared& s, uint32_t tid)
{
  x = wave_sum(x);
  y = wave_sum(y);
  __syncthreads();
  if ((tid & 63u) == 0) {
    s.red[tid >> 6][0] = x;
    s.red[tid >> 6][1] = y;
  }
  __syncthreads();
  return make_double2((s.red[0][0] + s.red[1][0]) + (s.red[2][0] + s.red[3][0]),
                      (s.red[0][1] + s.red[1][1]) + (s.red[2][1] + s.red[3][1]));
}

// Element n of the low-PAPR DM-RS of a PUSCH as its entry of the circle of desc.lp.circle points: r_{u,0}(n), M_zc = 6 nprb.
__device__ __forceinline__ uint32_t low_papr_dmrs_index(const PuschChestDesc& d, uint32_t n)
{
  if (d.nprb < 5u) {
    return low_papr_table_index(d.lp.phi[n]);
  }
  return d.nprb == 5u ? low_papr_zc30_index(d.lp.u, n) : low_papr_zc_index(d.lp.q, d.lp.n_zc, n);
}

// Pilot q of DM-RS symbol d (layer 0) on grid subcarrier 12 n + 2 k, PRB n = prbs[q / 6], k = q % 6.  Gold: r(6n + k), QPSK of
// the symbol's sequence from subcarrier 0 of the grid.  Low-PAPR: element q of the allocation's own sequence, amplitude 1.
template <PilotSource SRC>
__device__ __forceinline__ float2 pilot(const ChestShared& s, const PuschChestDesc& desc, uint32_t d, uint32_t q, uint32_t layer,
                                        uint32_t& subc)
{
  const uint32_t n = s.prbs[q / 6u], k = q % 6u;
  subc             = 12u * n + 2u * k; // also the Gold pilot's first bit: two bits per pilot, one pilot per two subcarriers
  float2 p;
  if (SRC == PILOT_GOLD) {
    p = qpsk_pilot(s.pil.gold.seq[d], subc);
  } else {
    p = unit_circle_libm(s.pil.lp_index[q], desc.lp.circle);
  }
  if (layer == 1 && (q & 1u)) { // w_f = -1 on the odd pilots of layer 1 (port 1001)
    p = make_float2(-p.x, -p.y);
  }
  return p;
}

template <PilotSource SRC>
__global__ __launch_bounds__(CHEST_THREADS) void pusch_chest_kernel(PuschChestLaunch p)
{
  __shared__ ChestShared s;
  const uint32_t       tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t       job = p.jobs[blockIdx.x];
  const uint32_t       ip = job >> 8, port = (job >> 4) & 15u, layer = job & 15u;
  const PuschChestDesc& d = p.desc[ip];
  const uint32_t       N = 6u * d.nprb, nd = d.nof_dmrs;

  for (uint32_t j = tid; j < d.nprb; j += CHEST_THREADS) {
    s.prbs[j] = p.prbs[d.prb_first + j];
  }
  for (uint32_t i = tid; i < 2048u; i += CHEST_THREADS) {
    s.u.tw[i] = p.twiddle[i];
  }
  if (SRC == PILOT_GOLD) {
    for (uint32_t dd = wave; dd < nd; dd += 4u) { // wave-uniform
      gold_sequence_wave(p.gold, p.x1_words, d.c_init[dd], d.nwords, s.pil.gold.seq[dd], s.pil.gold.scratch[wave], lane);
    }
  } else {
    for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
      s.pil.lp_index[q] = (uint16_t)low_papr_dmrs_index(d, q);
    }
  }
  __syncthreads();

  const uint32_t* grid  = p.grid + ((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[port]) * NRPHY_NSYMB * p.grid_nof_subc;
  float2*         A     = s.a + V_MARGIN;
  double          epre  = 0.0;
  float           cfo   = 0.f;
  // ---- LS estimates, EPRE, CFO (preprocess_pilots_and_cfo) --------------------------------------------------------------
  for (uint32_t dd = 0; dd != nd; ++dd) {
    const uint32_t* row = grid + (size_t)d.dmrs_symbol[dd] * p.grid_nof_subc;
    double          dr = 0.0, di = 0.0;
    for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
      uint32_t     k;
      const float2 pl = pilot<SRC>(s, d, dd, q, layer, k);
      const float2 y  = cbf16_to_float2(row[k]);
      epre += (double)exact::norm(y);
      const float2 ls = exact::mul_conj(y, pl);
      if (dd == 0) {
        A[q] = ls;
      } else if (dd == 1) {
        s.b[q] = ls;
        const float2 dot = exact::mul_conj(ls, A[q]); // dot_prod(LS1, LS0) = sum LS1 conj(LS0)
        dr += (double)dot.x;
        di += (double)dot.y;
      } else {
        const float2 r = phasor(__fmul_rn(__fmul_rn(-TWOPI_F, d.epoch[d.dmrs_symbol[dd]]), cfo));
        const float2 a = A[q], c = exact::cmul(ls, r);
        A[q]                     = make_float2(__fadd_rn(a.x, c.x), __fadd_rn(a.y, c.y));
      }
    }
    if (dd == 1) {
      const double2 dot   = block_sum2(dr, di, s, tid);
      const float   phase = (float)atan2((double)(float)dot.y, (double)(float)dot.x);
      cfo = __fdiv_rn(__fdiv_rn(phase, TWOPI_F), __fsub_rn(d.epoch[d.dmrs_symbol[1]], d.epoch[d.dmrs_symbol[0]]));
      const float2 r0 = phasor(__fmul_rn(__fmul_rn(-TWOPI_F, d.epoch[d.dmrs_symbol[0]]), cfo));
      const float2 r1 = phasor(__fmul_rn(__fmul_rn(-TWOPI_F, d.epoch[d.dmrs_symbol[1]]), cfo));
      for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
        const float2 a = exact::cmul(A[q], r0), c = exact::cmul(s.b[q], r1);
        A[q]           = make_float2(__fadd_rn(a.x, c.x), __fadd_rn(a.y, c.y));
      }
    }
    __syncthreads();
  }
  // Average and DM-RS-to-data gain.
  for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
    A[q] = make_float2(__fmul_rn(A[q].x, d.ls_scale), __fmul_rn(A[q].y, d.ls_scale));
  }
  __syncthreads();

  // ---- virtual pilots (add_v_pilots) and the FIR (convolution_same), the middle N outputs into b ------------------------
  const uint32_t nv = d.nof_v;
  if (tid < 2u * nv) {
    const uint32_t side = tid / nv, i = tid % nv;
    const float2   v    = A[side == 0 ? i : N - nv + i];
    const double   re = v.x, im = v.y;
    s.vp_abs[side][i] = (float)sqrt(re * re + im * im);
    s.vp_arg[side][i] = (float)atan2(im, re);
  }
  __syncthreads();
  if (tid < 2u) {
    virtual_pilots(s.vp_abs[tid], s.vp_arg[tid], nv, tid == 0 ? -(int)nv : (int)nv, tid == 0 ? A - nv : A + N);
  }
  __syncthreads();
  const uint32_t T = d.ntaps, mid = T / 2u;
  double         pw = 0.0;
  for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
    const float2* x  = A + q - mid;
    float2        acc = make_float2(0.f, 0.f);
    for (uint32_t i = 0; i != T; ++i) {
      const float h = d.taps[T - 1u - i];
      acc           = make_float2(__fadd_rn(acc.x, __fmul_rn(x[i].x, h)), __fadd_rn(acc.y, __fmul_rn(x[i].y, h)));
    }
    s.b[q] = acc;
    pw += (double)exact::norm(acc);
  }
  const double2 pe   = block_sum2(pw, epre, s, tid); // (also orders the writes of b)
  const float   rsrp = (float)(pe.x * (double)d.beta * (double)d.beta / (double)N);

  // ---- noise (estimate_noise) ------------------------------------------------------------------------------------------
  double ne = 0.0;
  for (uint32_t dd = 0; dd != nd; ++dd) {
    const uint32_t* row = grid + (size_t)d.dmrs_symbol[dd] * p.grid_nof_subc;
    const float2    r   = phasor(__fmul_rn(__fmul_rn(TWOPI_F, d.epoch[d.dmrs_symbol[dd]]), cfo));
    for (uint32_t q = tid; q < N; q += CHEST_THREADS) {
      uint32_t     k;
      const float2 pl = pilot<SRC>(s, d, dd, q, layer, k);
      const float2 y  = cbf16_to_float2(row[k]);
      const float2 f  = s.b[q];
      float2       e  = exact::cmul(make_float2(__fmul_rn(f.x, -d.beta), __fmul_rn(f.y, -d.beta)), pl);
      if (nd >= 2u) {
        e = exact::cmul(e, r);
      }
      e = make_float2(__fadd_rn(e.x, y.x), __fadd_rn(e.y, y.y));
      ne += (double)exact::norm(e);
    }
  }
  const double2 nz = block_sum2(ne, 0.0, s, tid);

  // ---- time alignment: |IDFT_4096|^2 of the filtered pilots at their grid subcarriers, bins [0, 144) and [3952, 4096) ------
  {
    float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
    const uint32_t n0 = tid < PUSCH_CHEST_TA_WINDOW ? tid : 4096u - TA_BINS + tid;
    const uint32_t b1 = tid + CHEST_THREADS, n1 = 4096u - TA_BINS + b1;
    const bool     two = b1 < TA_BINS;
    for (uint32_t j = 0; j != d.nprb; ++j) {
      const uint32_t m0 = 6u * s.prbs[j];
      uint32_t       i0 = (m0 * n0) & 2047u, i1 = (m0 * n1) & 2047u;
#pragma unroll
      for (uint32_t k = 0; k != 6; ++k) {
        const float2 f = s.b[6u * j + k];
        dft_accumulate(acc0, f, s.u.tw[i0]);
        if (two) {
          dft_accumulate(acc1, f, s.u.tw[i1]);
        }
        i0 = (i0 + n0) & 2047u;
        i1 = (i1 + n1) & 2047u;
      }
    }
    s.mag[tid] = exact::norm(acc0);
    if (two) {
      s.mag[b1] = exact::norm(acc1);
    }
  }
  __syncthreads(); // (the twiddles are dead from here on: u.out reuses them)

  // ---- linear interpolation (interpolator_linear_impl, offset 0, stride 2): half steps in parallel, the running sum serial
  float* half = reinterpret_cast<float*>(s.a); // two planes of N - 1
  for (uint32_t q = tid; q + 1u < N; q += CHEST_THREADS) {
    half[q]             = __fmul_rn(__fsub_rn(s.b[q + 1u].x, s.b[q].x), 0.5f);
    half[MAX_PILOTS + q] = __fmul_rn(__fsub_rn(s.b[q + 1u].y, s.b[q].y), 0.5f);
  }
  __syncthreads();
  if (tid < 2u) { // lane 0: real part, lane 1: imaginary part
    const float* h   = half + tid * MAX_PILOTS;
    float*       out = s.u.out[tid];
    float        v   = tid == 0 ? s.b[0].x : s.b[0].y;
    out[0]           = v;
    for (uint32_t i = 0; i + 1u < N; ++i) {
      const float j  = h[i];
      const float v1 = __fadd_rn(v, j);
      v              = __fadd_rn(v1, j);
      out[2u * i + 1u] = v1;
      out[2u * i + 2u] = v;
    }
    out[2u * N - 1u] = tid == 0 ? s.b[N - 1u].x : s.b[N - 1u].y;
  } else if (tid == 64u) { // meanwhile: the measurements
    float    best_d = -1.f, best_a = -1.f;
    uint32_t id = 0, ia = 0;
    for (uint32_t b = 0; b != PUSCH_CHEST_TA_WINDOW; ++b) {
      // Ascending, so the bin held is never above b and take_max's tie rule cannot fire: said aloud, the compiler keeps the
      // strict comparison only, as selects; left to find out, it branches per bin behind every LDS read.
      __builtin_assume(id <= b && ia <= b);
      take_max(best_d, id, s.mag[b], b);
      take_max(best_a, ia, s.mag[PUSCH_CHEST_TA_WINDOW + b], b);
    }
    const int ta_bins = ta_signed_bin(best_d, id, best_a, ia, PUSCH_CHEST_TA_WINDOW);
    const nrphy_pusch_chest_meas_t m = chest_measurements(rsrp, (float)(pe.y / (double)(N * nd)), (float)(nz.x / (double)(N * nd - 1u)),
                                                          d.beta, ta_bins, nd >= 2u, cfo, d.scs_hz);
    if (layer == 0) {
      p.noise_vars[(size_t)ip * NRPHY_MAX_PORTS + port] = m.noise_var;
    }
    if (p.meas != nullptr) {
      p.meas[((size_t)ip * NRPHY_MAX_PORTS + port) * PUSCH_CHEST_MAX_LAYERS + layer] = m;
    }
  } else if (tid >= 128u && tid < 128u + NRPHY_NSYMB) { // the per-symbol CFO phasors of the expand kernel
    const uint32_t l = tid - 128u;
    p.rot[(size_t)blockIdx.x * NRPHY_NSYMB + l] = nd >= 2u ? phasor(__fmul_rn(__fmul_rn(TWOPI_F, d.epoch[l]), cfo))
                                                             : make_float2(1.f, 0.f);
  }
  __syncthreads();
  uint32_t* row = p.rows + d.row_offset + (size_t)(port * d.nof_layers + layer) * 12u * d.nprb;
  for (uint32_t k = tid; k < 12u * d.nprb; k += CHEST_THREADS) {
    row[k] = to_cbf16(s.u.out[0][k], s.u.out[1][k]);
  }
}

} // namespace
} // namespace nrphy
