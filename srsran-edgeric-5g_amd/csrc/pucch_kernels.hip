// PUCCH format 0 and format 1 receivers for gfx950.
//
// Replaces pucch_processor_impl::process for format0_configuration and format1_configuration
// (R/lib/phy/upper/channel_processors/pucch_processor_impl.cpp:29-129): pucch_detector_format0::detect
// (pucch_detector_format0.cpp:66-202); dmrs_pucch_processor_format1_impl::estimate (dmrs_pucch_processor_format1_impl.cpp:158-222)
// on port_channel_estimator_average_impl::compute with the `mean` smoothing strategy and CFO compensation off, followed by
// pucch_detector_format1::detect (pucch_detector_format1.cpp:92-293) and channel_estimate::get_channel_state_information.
//
// A PUCCH is at most 4 ports x 14 symbols x 12 RE, so the split is the opposite of the PUSCH estimator's: one wavefront per
// PUCCH, four per workgroup, no LDS, no barrier, no scratch.  The descriptor index is made scalar (readfirstlane), so the
// descriptor is read with scalar loads.  A (port, symbol) row of the PRB is 48 bytes at a multiple of 48: three 16-byte loads.
//
//   format 0: lane = candidate * 8 + symbol * 4 + port.  A lane correlates its row with its candidate's sequence (12 RE, in
//             order, double sums); sum_corr and sum_noise_var are then added in float in the reference's order (symbol outer, port
//             inner) from the lanes of the candidate, and the candidates compared in table order.
//   format 1: estimation on lane = port * 8 + hop * 4 + chunk (4 RE of the row per lane, the DM-RS symbols of the hop in
//             order), sums over the row folded over the 4 lanes of a group; the estimate (one value per port and hop) is written
//             by lane = port * nof_symbols + symbol; detection on lane = data symbol * 4 + chunk, every RE equalised over the
//             ports with the equaliser of equalize_device.h, the three sums folded with wave_sum.
// Every reduction is a per-lane double partial sum folded in a fixed order and rounded once: two runs give the same bytes.
// atan2 and log10 are evaluated in double and rounded once.  Contraction is off.
//
// The time alignment is 0 by construction (include/mi355_nrphy.h says why): no transform is computed.
#include "bits_device.h"
#include "equalize_device.h"

#include <hip/hip_runtime.h>

namespace nrphy {
namespace {

constexpr uint32_t PUCCH_WAVES = 4;    // PUCCHs per workgroup
constexpr float    THRESHOLD   = 4.0f;
constexpr uint32_t MAX_DMRS    = 7;    // DM-RS symbols of a hop: 14 symbols without hopping

// r_uv^alpha(n), length 12: the base sequence times the cyclic shift (low_papr_sequence_generator_impl::generate).
__device__ __forceinline__ float2 low_papr(const PucchTables& t, uint32_t u, uint32_t alpha, uint32_t n)
{
  return exact::cmul(t.base[u][n], t.shift[(2u * alpha * n) % 24u]);
}

// Sum over the 4 lanes of a group in a fixed order; every lane of the group gets the result.
__device__ __forceinline__ double group_sum4(double x)
{
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  return x;
}

__device__ __forceinline__ uint32_t word_of(const uint4& w, uint32_t i)
{
  return i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w;
}

__device__ __forceinline__ const uint32_t* row_of(const PucchLaunch& p, const PucchDesc& d, uint32_t port, uint32_t symbol, uint32_t prb)
{
  return p.grid + (((size_t)d.grid_index * p.grid_nof_ports + d.rx_ports[port]) * NRPHY_NSYMB + symbol) * p.grid_nof_subc +
         (size_t)NRPHY_NRE * prb;
}

__device__ __forceinline__ void write_result(const PucchLaunch& p, uint32_t ip, uint32_t status, uint32_t a0, uint32_t a1, uint32_t sr,
                                             float metric, float sinr, float rsrp, float epre, float cfo_hz)
{
  nrphy_pucch_result_t r;
  r.status           = status;
  r.harq_ack[0]      = a0;
  r.harq_ack[1]      = a1;
  r.sr               = sr;
  r.detection_metric = metric;
  r.sinr_dB          = sinr;
  r.rsrp_dB          = rsrp;
  r.epre_dB          = epre;
  r.time_alignment_s = 0.f;
  r.cfo_hz           = cfo_hz;
  p.result[ip]       = r;
}

// The five dictionaries of pucch_detector_format0.cpp:42-64, entry = m_cs | sr << 4 | ack0 << 5 | ack1 << 6, in table order.
__device__ __forceinline__ uint32_t format0_entry(uint32_t nof_harq_ack, uint32_t sr_opportunity, uint32_t i)
{
  constexpr uint32_t E = 0x10; // SR bit
  constexpr uint32_t A = 0x20, B = 0x40;
  if (nof_harq_ack == 0) {
    return 0u | E;
  }
  // Four 8-bit entries per word, picked with a shift: no array is indexed at run time.
  if (nof_harq_ack == 1) {
    constexpr uint32_t WITH_SR = 0u | (6u | A) << 8 | (3u | E) << 16 | (9u | E | A) << 24;
    constexpr uint32_t NO_SR   = 0u | (6u | A) << 8;
    return sr_opportunity ? (WITH_SR >> (8u * (i & 3u))) & 0xFFu : (NO_SR >> (8u * (i & 1u))) & 0xFFu;
  }
  constexpr uint32_t FOUR = 0u | (3u | B) << 8 | (6u | A | B) << 16 | (9u | A) << 24;
  const uint32_t     e    = (FOUR >> (8u * (i & 3u))) & 0xFFu;
  return i < 4u ? e : (e + 1u) | E;
}

__device__ void pucch_format0(const PucchLaunch& p, const PucchDesc& d, uint32_t ip, uint32_t lane)
{
  const PucchTables& t     = *p.tables;
  const uint32_t     P = d.nof_rx_ports, ns = d.nof_symbols;
  const uint32_t     ncand = d.nof_harq_ack == 0 ? 1u : (d.nof_harq_ack == 1 ? 2u : 4u) << d.sr_opportunity;
  const uint32_t     cand = lane >> 3, sym = (lane >> 2) & 1u, port = lane & 3u;
  const bool         active = cand < ncand && sym < ns && port < P;
  float              corr = 0.f, nvc = 0.f, avg_y = 0.f;
  if (active) {
    const uint32_t m_cs  = format0_entry(d.nof_harq_ack, d.sr_opportunity, cand) & 15u;
    const uint32_t alpha = (d.alpha[sym] + m_cs) % NRPHY_NRE;
    const uint4*   row   = reinterpret_cast<const uint4*>(row_of(p, d, port, d.first_symbol + sym, d.prb[sym]));
    const uint4    w[3]  = {row[0], row[1], row[2]};
    double         pw_l = 0.0, pw_y = 0.0, sr = 0.0, si = 0.0;
#pragma unroll
    for (uint32_t k = 0; k != NRPHY_NRE; ++k) {
      const float2 y   = cbf16_to_float2(word_of(w[k >> 2], k & 3u));
      const float2 lse = exact::mul_conj(y, low_papr(t, d.u, alpha, k));
      pw_y += (double)exact::norm(y);
      pw_l += (double)exact::norm(lse);
      sr += (double)lse.x;
      si += (double)lse.y;
    }
    const float  avg_pwr = (float)(pw_l / 12.0);
    const float2 mean    = make_float2(__fdiv_rn((float)sr, 12.0f), __fdiv_rn((float)si, 12.0f));
    corr                 = exact::norm(mean);
    const float diff     = __fsub_rn(avg_pwr, corr);
    nvc                  = __fmul_rn(diff > 0.f ? diff : 0.f, corr);
    avg_y                = (float)(pw_y / 12.0);
  }
  // The reference's accumulation order: symbol outer, port inner.
  float sum_corr = 0.f, sum_nv = 0.f, epre = 0.f;
  for (uint32_t s = 0; s != ns; ++s) {
    for (uint32_t q = 0; q != P; ++q) {
      const uint32_t src = s * 4u + q;
      sum_corr           = __fadd_rn(sum_corr, __shfl(corr, (lane & ~7u) + src));
      sum_nv             = __fadd_rn(sum_nv, __shfl(nvc, (lane & ~7u) + src));
      epre               = __fadd_rn(epre, __shfl(avg_y, src));
    }
  }
  epre               = __fdiv_rn(epre, (float)(ns * P));
  const float metric = is_normal(sum_nv) ? __fdiv_rn(__fmul_rn(sum_corr, sum_corr), sum_nv) : 0.f;
  float       best = 0.f, best_rsrp = 0.f;
  uint32_t    msg = 0;
  for (uint32_t c = 0; c != ncand; ++c) {
    const float m = __shfl(metric, c * 8u), sc = __shfl(sum_corr, c * 8u);
    if (m > best) {
      best      = m;
      best_rsrp = sc;
      msg       = format0_entry(d.nof_harq_ack, d.sr_opportunity, c);
    }
  }
  if (lane == 0) {
    write_result(p, ip, best > THRESHOLD ? NRPHY_PUCCH_STATUS_VALID : NRPHY_PUCCH_STATUS_INVALID, (msg >> 5) & 1u, (msg >> 6) & 1u,
                 (msg >> 4) & 1u, best, to_dB(best), to_dB(best_rsrp), to_dB(epre), __builtin_nanf(""));
  }
  if (p.meas != nullptr && lane < NRPHY_MAX_PORTS) {
    nrphy_pusch_chest_meas_t z = {};
    p.meas[(size_t)ip * NRPHY_MAX_PORTS + lane] = z;
  }
}

__device__ void pucch_format1(const PucchLaunch& p, const PucchDesc& d, uint32_t ip, uint32_t lane)
{
  const PucchTables& t  = *p.tables;
  const uint32_t     P = d.nof_rx_ports, ns = d.nof_symbols, s0 = d.first_symbol;
  const uint32_t     half   = d.hopping ? ns / 2u : ns; // symbols of the first hop
  const uint32_t     nd0    = (half + 1u) / 2u;         // DM-RS symbols (even symbols of the allocation) of the first hop
  const uint32_t     nd_all = (ns + 1u) / 2u, nd1 = nd_all - nd0;

  // ---- estimation: lane = port * 8 + hop * 4 + chunk -----------------------------------------------------------------------
  float    epre_hop = 0.f, rsrp_hop = 0.f, noise_hop = 0.f, cfo_hop = 0.f;
  uint32_t h_word   = 0;
  {
    const uint32_t port = lane >> 3, hop = (lane >> 2) & 1u, chunk = lane & 3u;
    const bool     group  = lane < 32u && port < P && (hop == 0 || d.hopping != 0);
    const bool     active = group && chunk < 3u;
    const uint32_t nd = hop ? nd1 : nd0, j0 = hop ? nd0 : 0u;
    uint4          yw[MAX_DMRS] = {};
    float2         z[MAX_DMRS][4] = {};
    float2         lse[4] = {};
    double         dr = 0.0, di = 0.0;
#pragma unroll
    for (uint32_t j = 0; j != MAX_DMRS; ++j) {
      if (j < nd) {                     // uniform over the group
        double pw = 0.0;
        if (active) {
          const uint32_t off   = 2u * (j0 + j);
          const uint32_t alpha = d.alpha[off];
          const float2   w     = t.occ[nd - 1u][d.occ][j];
          yw[j] = reinterpret_cast<const uint4*>(row_of(p, d, port, s0 + off, d.prb[hop]))[chunk];
#pragma unroll
          for (uint32_t i = 0; i != 4; ++i) {
            const float2 y = cbf16_to_float2(word_of(yw[j], i));
            z[j][i]        = exact::cmul(low_papr(t, d.u, alpha, 4u * chunk + i), w); // z = w_i(m) r_uv^alpha
            const float2 ls = exact::mul_conj(y, z[j][i]);
            pw += (double)exact::norm(y);
            if (j == 0) {
              lse[i] = ls;
            } else {
              if (j == 1) { // dot_prod(LS1, LS0) = sum LS1 conj(LS0)
                const float2 dot = exact::mul_conj(ls, lse[i]);
                dr += (double)dot.x;
                di += (double)dot.y;
              }
              lse[i] = make_float2(__fadd_rn(lse[i].x, ls.x), __fadd_rn(lse[i].y, ls.y));
            }
          }
        }
        epre_hop = __fadd_rn(epre_hop, __fmul_rn((float)(group_sum4(pw) / 12.0), 12.0f));
      }
    }
    dr = group_sum4(dr);
    di = group_sum4(di);
    if (nd >= 2u) {
      const float phase = (float)atan2((double)(float)di, (double)(float)dr);
      cfo_hop           = __fdiv_rn(__fdiv_rn(phase, TWOPI_F), d.cfo_dt[hop]);
    }
    // Average (DM-RS-to-data gain 1), then the `mean` smoothing: one value for the hop.
    const float scale = __fdiv_rn(1.0f, __fmul_rn((float)nd, 1.0f));
    double      mr = 0.0, mi = 0.0;
#pragma unroll
    for (uint32_t i = 0; i != 4; ++i) {
      mr += (double)__fmul_rn(lse[i].x, scale);
      mi += (double)__fmul_rn(lse[i].y, scale);
    }
    const float2 h = make_float2((float)(group_sum4(mr) / 12.0), (float)(group_sum4(mi) / 12.0));
    rsrp_hop       = __fmul_rn(__fmul_rn(exact::norm(h), 12.0f), (float)nd);
    h_word         = to_cbf16(h.x, h.y);
    // Noise (noise_no_cfo): |rx - h z|^2 per DM-RS symbol.
    const float2 neg_h = make_float2(-h.x, -h.y);
#pragma unroll
    for (uint32_t j = 0; j != MAX_DMRS; ++j) {
      if (j < nd) {
        double pw = 0.0;
        if (active) {
#pragma unroll
          for (uint32_t i = 0; i != 4; ++i) {
            const float2 y = cbf16_to_float2(word_of(yw[j], i));
            const float2 e = exact::cmul(neg_h, z[j][i]);
            pw += (double)exact::norm(make_float2(__fadd_rn(e.x, y.x), __fadd_rn(e.y, y.y)));
          }
        }
        noise_hop = __fadd_rn(noise_hop, __fmul_rn((float)(group_sum4(pw) / 12.0), 12.0f));
      }
    }
    if (!group) {
      epre_hop = rsrp_hop = noise_hop = cfo_hop = 0.f;
      h_word = 0;
    }
  }

  // ---- the estimate: lane = port * nof_symbols + symbol, the hop's value on the 12 subcarriers of the hop's PRB -------------
  {
    const uint32_t port = lane / ns, off = lane % ns;
    const uint32_t hop  = (d.hopping != 0 && off >= half) ? 1u : 0u;
    const uint32_t w    = __shfl(h_word, (port & 3u) * 8u + hop * 4u);
    if (p.ch != nullptr && port < P) {
      uint32_t* dst = p.ch + d.ce_offset + ((size_t)port * NRPHY_NSYMB + s0 + off) * p.grid_nof_subc + (size_t)NRPHY_NRE * d.prb[hop];
      if ((((uintptr_t)dst) & 15u) == 0) {
        const uint4 v = make_uint4(w, w, w, w);
        reinterpret_cast<uint4*>(dst)[0] = v;
        reinterpret_cast<uint4*>(dst)[1] = v;
        reinterpret_cast<uint4*>(dst)[2] = v;
      } else {
#pragma unroll
        for (uint32_t k = 0; k != NRPHY_NRE; ++k) {
          dst[k] = w;
        }
      }
    }
  }

  // ---- hops and ports merged (port_channel_estimator_average_impl::compute, get_channel_state_information) ------------------
  uint32_t hw[2][NRPHY_MAX_PORTS] = {}; // [hop][port]
  float    nv[NRPHY_MAX_PORTS]    = {};
  CsiMerge csi;
  const float nof_pilots = (float)(NRPHY_NRE * nd_all), nof_pilots_1 = (float)(NRPHY_NRE * nd_all - 1u);
#pragma unroll
  for (uint32_t q = 0; q != NRPHY_MAX_PORTS; ++q) {
    const uint32_t a = q * 8u, b = q * 8u + 4u;
    hw[0][q]         = __shfl(h_word, a);
    hw[1][q]         = __shfl(h_word, b);
    float epre = __shfl(epre_hop, a), rsrp = __shfl(rsrp_hop, a), noise = __shfl(noise_hop, a);
    const float e1 = __shfl(epre_hop, b), r1 = __shfl(rsrp_hop, b), n1 = __shfl(noise_hop, b);
    const float c0 = __shfl(cfo_hop, a), c1 = __shfl(cfo_hop, b);
    if (d.hopping != 0) {
      epre  = __fadd_rn(epre, e1);
      rsrp  = __fadd_rn(rsrp, r1);
      noise = __fadd_rn(noise, n1);
    }
    const bool  has0 = nd0 >= 2u, has1 = d.hopping != 0 && nd1 >= 2u;
    const float cfo  = has0 && has1 ? __fdiv_rn(__fadd_rn(c0, c1), 2.0f) : has0 ? c0 : c1;
    rsrp             = __fdiv_rn(rsrp, nof_pilots);
    epre             = __fdiv_rn(epre, nof_pilots);
    noise            = __fdiv_rn(noise, nof_pilots_1);
    const float min_noise = __fdiv_rn(rsrp, 1e10f);
    const float noise_var = min_noise < noise ? noise : min_noise;
    const float snr       = noise_var != 0.f ? __fdiv_rn(rsrp, noise_var) : 1000.f;
    const float cfo_hz    = has0 || has1 ? __fmul_rn(__fmul_rn(cfo, (float)d.scs_khz), 1000.f) : __builtin_nanf("");
    if (q < P) {
      nv[q] = noise_var;
      csi.add(q, noise_var, rsrp, epre, snr, 0.f, cfo_hz);
    }
    if (p.meas != nullptr && lane == q) {
      nrphy_pusch_chest_meas_t m = {};
      if (q < P) {
        m.noise_var = noise_var;
        m.rsrp      = rsrp;
        m.epre      = epre;
        m.snr       = snr;
        m.cfo_hz    = cfo_hz;
      }
      p.meas[(size_t)ip * NRPHY_MAX_PORTS + q] = m;
    }
  }

  // ---- detection: lane = data symbol * 4 + chunk ----------------------------------------------------------------------------
  const uint32_t ndata = ns / 2u, npre = d.hopping ? ns / 4u : ndata;
  double         sr = 0.0, si = 0.0, sv = 0.0;
  {
    const uint32_t dsym = lane >> 2, chunk = lane & 3u;
    if (dsym < ndata && chunk < 3u) {
      const uint32_t off = 2u * dsym + 1u;
      const uint32_t hop = dsym < npre ? 0u : 1u; // the second hop's PRB and estimate
      const float2   w   = dsym < npre ? t.occ[npre - 1u][d.occ][dsym] : t.occ[ndata - npre - 1u][d.occ][dsym - npre];
      const float2   w_star = make_float2(w.x, -w.y);
      const uint32_t alpha  = d.alpha[off];
      const float    nv_max = max_noise(nv, P);
      uint4          yw[NRPHY_MAX_PORTS] = {};
      uint32_t       h[2][NRPHY_MAX_PORTS] = {};
#pragma unroll
      for (uint32_t q = 0; q != NRPHY_MAX_PORTS; ++q) {
        if (q < P) {
          yw[q]   = reinterpret_cast<const uint4*>(row_of(p, d, q, s0 + off, d.prb[hop]))[chunk];
          h[0][q] = hop ? hw[1][q] : hw[0][q];
        }
      }
#pragma unroll
      for (uint32_t i = 0; i != 4; ++i) {
        uint32_t y[NRPHY_MAX_PORTS];
#pragma unroll
        for (uint32_t q = 0; q != NRPHY_MAX_PORTS; ++q) {
          y[q] = word_of(yw[q], i);
        }
        float2 x[2];
        float  v[2];
        equalize_re(NRPHY_EQ_ZF, 1u, P, y, h, nv, nv_max, 1.0f, x, v);
        const float2 r = low_papr(t, d.u, alpha, 4u * chunk + i);
        const float2 e = exact::cmul(exact::cmul(x[0], w_star), make_float2(r.x, -r.y));
        sr += (double)e.x;
        si += (double)e.y;
        sv += (double)v[0];
      }
    }
  }
  sr = wave_sum(sr);
  si = wave_sum(si);
  sv = wave_sum(sv);
  if (lane == 0) {
    const float  nre = (float)(NRPHY_NRE * ndata);
    const float2 det = make_float2(__fdiv_rn((float)sr, nre), __fdiv_rn((float)si, nre));
    const float  eq_noise_var = __fdiv_rn((float)(sv / (double)(NRPHY_NRE * ndata)), nre);
    // detect_bits
    float    m1 = __fadd_rn(det.x, det.y), m2 = __fsub_rn(det.x, det.y);
    uint32_t bits = m1 > 0.f ? 0u : 3u;
    const uint32_t bits2 = m2 > 0.f ? 2u : 1u;
    m1 = fabsf(m1);
    m2 = fabsf(m2);
    if (d.nof_harq_ack > 1u && m2 > m1) {
      bits = bits2;
    }
    const float metric = __fdiv_rn(exact::norm(det), eq_noise_var);
    const bool  ok     = metric > THRESHOLD;
    uint32_t    status = NRPHY_PUCCH_STATUS_INVALID;
    if (ok) {
      status = d.nof_harq_ack > 0u || (bits & 1u) == 0u ? NRPHY_PUCCH_STATUS_VALID : NRPHY_PUCCH_STATUS_UNKNOWN;
    }
    write_result(p, ip, status, d.nof_harq_ack > 0u ? bits & 1u : 0u, d.nof_harq_ack > 1u ? (bits >> 1) & 1u : 0u, 0u,
                 __fdiv_rn(metric, THRESHOLD), csi.sinr_dB(), csi.rsrp_dB(P), csi.epre_dB(P), csi.cfo_hz);
  }
}

__global__ __launch_bounds__(PUCCH_WAVES * WAVE) void pucch_kernel(PucchLaunch p)
{
  const uint32_t ip = __builtin_amdgcn_readfirstlane(blockIdx.x * PUCCH_WAVES + (threadIdx.x >> 6));
  if (ip >= p.n) {
    return;
  }
  const PucchDesc& d    = p.desc[ip];
  const uint32_t   lane = threadIdx.x & 63u;
  if (d.format == NRPHY_PUCCH_FORMAT_0) {
    pucch_format0(p, d, ip, lane);
  } else {
    pucch_format1(p, d, ip, lane);
  }
}

} // namespace

hipError_t launch_pucch(const PucchLaunch& p, hipStream_t stream)
{
  if (p.n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pucch_kernel, dim3((p.n + PUCCH_WAVES - 1) / PUCCH_WAVES), dim3(PUCCH_WAVES * WAVE), 0, stream, p);
  return hipGetLastError();
}

} // namespace nrphy
